"""--fetch-codec q8delta without a GPU (parallel/fetchq8.py): the scheme on the torch path (error
bound per round, the worker mirror bit for bit, exact convergence on a frozen arena, NaN / Inf
blocks), the configuration rules, a world-2 gloo job, and the compiler's resource remarks for the
encode kernel."""
import os

import pytest
import torch

from psx.parallel import fetchq8 as F
from psx.parallel import q8 as Q
from psx.utils.config import PSConfig

from .test_kernel_resources_cpu import ROOT, _hipcc, _tool
from .test_ps_cpu import TINY, _spawn

SIZES = [255, 256, 257, 4097, 100003]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _block_amax(d, n):
    """max |d| of every element's block (tail block zero-filled), per element, fp64."""
    return Q._blocks(d).abs().amax(dim=1).repeat_interleave(Q.BLOCK)[:n].double()


@pytest.mark.parametrize("n", SIZES)
def test_scheme_bound_mirror_and_convergence(n):
    """60 rounds of arena -= lr * noise (about 1 % of the elements step 10x as far, so their blocks
    get a coarse scale). After every fetch, in fp64 and element-wise,
        |arena - shadow| <= amax_block / 254 * (1 + 1e-6) + (|arena| + |shadow|) * 2^-23:
    half a quantum of the block plus the roundings of the subtraction and of the add, so a rounding
    mode or a contracted multiply-add trips it. A mirror that sees only the payloads equals the
    shadow bit for bit after every round. Then the arena is frozen: within 8 further fetches
    shadow == arena exactly (the torch path takes 3 to 4 here)."""
    g = torch.Generator().manual_seed(1234 + n)
    arena = torch.randn(n, generator=g) * 0.05
    shadow = arena.clone()
    mirror = arena.clone()
    payload = Q.empty_payload(n, "cpu")
    lr = 0.01
    worst = 0.0
    for _ in range(60):
        step = torch.randn(n, generator=g) * 0.1
        step = torch.where(torch.rand(n, generator=g) < 0.01, step * 10.0, step)
        arena -= lr * step
        amax = _block_amax(arena - shadow, n)
        F.encode_into(arena, shadow, payload, n)
        F.apply(payload, mirror, n)
        assert _same(mirror, shadow)
        err = (arena.double() - shadow.double()).abs()
        bound = amax / 254.0 * (1 + 1e-6) + (arena.double().abs() + shadow.double().abs()) * 2.0 ** -23
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (n, worst)
    print(f"n={n}: worst |arena - shadow| / bound over 60 rounds = {worst:.6f}")
    took = None
    for k in range(1, 9):
        F.encode_into(arena, shadow, payload, n)
        F.apply(payload, mirror, n)
        assert _same(mirror, shadow)
        if _same(shadow, arena):
            took = k
            break
    print(f"n={n}: frozen arena reached exactly after {took} fetches")
    assert took is not None, n


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_block_goes_nan_alone(bad):
    n = 4097
    g = torch.Generator().manual_seed(7)
    base = torch.randn(n, generator=g) * 0.05
    arena = base + torch.randn(n, generator=g) * 1e-3
    ref_shadow, ref_payload = base.clone(), Q.empty_payload(n, "cpu")
    F.encode_into(arena, ref_shadow, ref_payload, n)
    arena_bad = arena.clone()
    arena_bad[300] = bad  # block 1
    arena_bad[4096] = bad  # the one-element tail block
    shadow, mirror, payload = base.clone(), base.clone(), Q.empty_payload(n, "cpu")
    F.encode_into(arena_bad, shadow, payload, n)
    F.apply(payload, mirror, n)
    _, scales, q = Q.views(payload, n)
    assert bool(scales[1].isnan()) and bool(scales[16].isnan()) and int(q[256:512].abs().sum()) == 0
    for t in (shadow, mirror):
        assert bool(t[256:512].isnan().all()) and bool(t[4096:].isnan().all())
        assert _same(t[:256], ref_shadow[:256]) and _same(t[512:4096], ref_shadow[512:4096])
    # it stays NaN on both sides, the other blocks go on
    F.encode_into(arena, shadow, payload, n)
    F.apply(payload, mirror, n)
    assert bool(shadow[256:512].isnan().all()) and bool(mirror[256:512].isnan().all())
    assert bool(shadow[:256].isfinite().all()) and _same(mirror[:256], shadow[:256])


def test_zero_delta_and_subrange():
    n = 4097
    g = torch.Generator().manual_seed(3)
    base = torch.randn(n, generator=g)
    arena = base.clone()
    arena[256:] += torch.randn(n - 256, generator=g) * 1e-3  # block 0 unchanged
    whole_s, whole_p = base.clone(), Q.empty_payload(n, "cpu")
    F.encode_into(arena, whole_s, whole_p, n)
    _, scales, q = Q.views(whole_p, n)
    assert float(scales[0]) == 0.0 and int(q[:256].abs().sum()) == 0 and _same(whole_s[:256], base[:256])
    part_s, part_p = base.clone(), Q.empty_payload(n, "cpu")
    F.encode_into(arena, part_s, part_p, n, off=512, cnt=1024)
    assert _same(part_s[512:1536], whole_s[512:1536]) and _same(part_s[:512], base[:512])
    assert _same(part_s[1536:], base[1536:])
    _, ps, pq = Q.views(part_p, n)
    assert torch.equal(pq[512:1536], q[512:1536]) and _same(ps[2:6], scales[2:6])
    assert int(pq[:512].abs().sum()) == 0 and int(pq[1536:].abs().sum()) == 0
    with pytest.raises(ValueError):
        F.encode_into(arena, part_s, part_p, n, off=100)


# ---------------------------------------------------------------------------- configuration
@pytest.mark.parametrize("kw", [
    dict(), dict(topology="dedicated"), dict(dtype="bf16"), dict(codec="sign1"), dict(codec="q8"), dict(codec="topk"),
    dict(codec="none"), dict(optimizer="lars"), dict(optimizer="adamw"), dict(optimizer="lamb"), dict(sync_steps=4),
    dict(overlap=False)])
def test_config_accepts(kw):
    cfg = PSConfig(mode="sync", fetch_codec="q8delta", **kw).validate()
    assert cfg.fetch_codec == "q8delta"


@pytest.mark.parametrize("kw,why", [(dict(mode="async"), "sync"), (dict(topology="sharded"), "sharded"),
                                    (dict(overlap=True), "overlap")])
def test_config_rejects_with_reason(kw, why):
    base = dict(mode="sync", fetch_codec="q8delta")
    base.update(kw)
    with pytest.raises(ValueError, match=r"q8delta.*" + why):
        PSConfig(**base).validate()


def test_config_cli_choice():
    from psx.utils.config import parse

    assert parse(["--mode", "sync", "--fetch-codec", "q8delta"]).fetch_codec == "q8delta"


def test_paths_that_decline():
    from psx.parallel import elastic
    from psx.parallel.codec import weight_image_enabled

    class _T:
        native = True

    cfg = PSConfig(mode="sync", fetch_codec="q8delta", topology="dedicated").validate()
    assert cfg.resolve_overlap(4) is False and cfg.overlap is False
    assert elastic.enabled(cfg, _T(), 4) is False
    assert weight_image_enabled(cfg) is False
    plain = PSConfig(mode="sync", fetch_codec="fp32", topology="dedicated").validate()
    plain.resolve_overlap(4)
    assert elastic.enabled(plain, _T(), 4) is True  # the codec is what declines


# ---------------------------------------------------------------------------- loopback and gloo
def test_loopback_workers_hold_the_shadow():
    """run_local, W = 2, CPU: every simulated worker ends on the server's shadow, the first fetch
    is a keyframe per worker and every later one a payload."""
    from psx.parallel.runner import build_state, run_local

    cfg = PSConfig(model="resnet_tiny", batch_size=8, epochs=1, train_samples=96, eval_every=0, verbose=0,
                   use_graph=False, lr=0.05, mode="sync", workers=2, max_steps=3, fetch_codec="q8delta").validate()
    res = run_local(cfg, log=lambda *a, **k: None)
    srv = res["server"]
    n = build_state(cfg)[1].arena_numel
    assert srv["global_steps_completed"] == 3
    assert srv["fetch_shadow_sha256"] and srv["fetch_shadow_sha256"] != srv["final_param_sha256"]
    assert [w["local_arena_sha256"] for w in res["workers"]] == [srv["fetch_shadow_sha256"]] * 2
    assert srv["bytes_fetched"] == 2 * (4 * n + 2 * Q.payload_bytes(n))


def test_dist_sync_q8delta_gloo():
    """World 2 over gloo, 3 rounds: rank 1 ends on the bits of rank 0's shadow, and the fetches
    moved one fp32 keyframe and two payloads to the one remote worker."""
    from psx.parallel.runner import build_state

    args = ["--mode", "sync", "--fetch-codec", "q8delta"] + TINY + ["--max-steps", "3", "--eval-every", "0"]
    recs, _ = _spawn(2, args)
    srv = [r for r in recs if r["type"] == "SERVER_FINAL_METRICS"][0]
    wks = {r["worker_id"]: r for r in recs if r["type"] == "WORKER_FINAL_METRICS"}
    assert srv["global_steps_completed"] == 3 and sorted(wks) == [0, 1]
    assert wks[1]["local_arena_sha256"] == srv["fetch_shadow_sha256"] == wks[0]["local_arena_sha256"]
    cfg = PSConfig(model="resnet_tiny").validate()
    n = build_state(cfg)[1].arena_numel
    assert srv["bytes_fetched"] == 4 * n + 2 * Q.payload_bytes(n)


# ---------------------------------------------------------------------------- compiler resources
def test_encode_kernel_no_scratch_no_spills():
    if not os.path.exists(_hipcc()):
        pytest.skip("hipcc is not installed")
    rows = [r for r in _tool().kernel_resources(os.path.join(ROOT, "csrc", "kernels", "q8.hip"))
            if "fetchq8_encode_kernel" in r["kernel"]]
    assert len(rows) == 2, rows  # the 16-byte form and the element-wise form
    for r in rows:
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, r
