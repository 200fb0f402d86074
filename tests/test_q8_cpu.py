"""Block-scaled int8 gradient codec (parallel/q8.py) on the CPU path: wire format, the fixed
arithmetic's properties, error feedback, server decode, and end-to-end PS runs (loopback + gloo)
with --codec q8."""
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel import q8 as Q
from psx.parallel.runner import run_local
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

from .test_ps_cpu import TINY, _spawn, tiny_cfg

FMAX = torch.finfo(torch.float32).max


@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_format(n):
    nblk = -(-n // 256)
    pad = lambda x: -(-x // 16) * 16  # noqa: E731
    assert Q.num_blocks(n) == nblk
    assert Q.section_offsets(n) == (16, 16 + pad(4 * nblk), 16 + pad(4 * nblk) + pad(n))
    assert Q.payload_bytes(n) == 16 + pad(4 * nblk) + pad(n)
    e = Q.empty_payload(n, "cpu")
    assert e.dtype == torch.uint8 and e.numel() == Q.payload_bytes(n)
    assert bytes(e[:4].tolist()) == b"Q8B1"
    assert e[:16].view(torch.int32).tolist() == [Q.MAGIC, n, 256, nblk]
    assert not e[16:].any() and not Q.decode(e, n).any()
    c = Q.Q8Codec(n)
    assert c.nbytes == Q.payload_bytes(n)
    p = c.encode(torch.randn(n))
    hdr, scales, q = Q.views(p, n)
    assert hdr.tolist() == [Q.MAGIC, n, 256, nblk] and scales.numel() == nblk and q.numel() == n
    assert scales.data_ptr() - p.data_ptr() == 16 and q.data_ptr() - p.data_ptr() == 16 + pad(4 * nblk)
    # the padding of both sections stays zero
    assert not p[16 + 4 * nblk:16 + pad(4 * nblk)].any() and not p[16 + pad(4 * nblk) + n:].any()


def check_step(acc: torch.Tensor, payload: torch.Tensor, resid: torch.Tensor, n: int):
    """The encode properties of one step, computed here in torch from the step's fp32 input
    ``acc = resid_before + float(g)`` (CPU tensors) — not through the codec's own reference."""
    hdr, scales, q = Q.views(payload, n)
    nblk = -(-n // 256)
    assert hdr.tolist() == [Q.MAGIC, n, 256, nblk]
    a = torch.cat([acc, acc.new_zeros(nblk * 256 - n)]).view(nblk, 256)
    nonfinite = ~(a.abs() <= FMAX)
    bad = nonfinite.any(1)
    amax = torch.where(nonfinite, torch.zeros_like(a), a.abs()).amax(1)
    good = ~bad
    # scale == amax / 127 exactly; |q| <= 127
    assert torch.equal(scales[good], (amax / torch.full_like(amax, 127.0))[good])
    assert int(q.to(torch.int32).abs().max()) <= 127
    sc = scales.repeat_interleave(256)[:n]
    deq = q.to(torch.float32) * sc
    ok = good.repeat_interleave(256)[:n]
    # |acc - deq| <= half a step (three roundings of <= 2^-24 on a value of <= 127 steps)
    assert bool(((acc - deq).abs()[ok] <= 0.5 * sc[ok] * (1 + 1e-4)).all())
    # error feedback is exact: resid + deq == acc
    assert torch.equal((resid + deq)[ok], acc[ok])
    # an all-zero block: scale 0, q 0, finite decode
    zero = good & (amax == 0)
    zb = zero.repeat_interleave(256)[:n]
    assert not scales[zero].any() and not q[zb].any()
    dec = Q.decode(payload.clone(), n)
    assert torch.equal(dec[ok], deq[ok]) and bool(torch.isfinite(dec[ok]).all())
    # a block holding NaN or Inf: scale NaN, q 0, non-finite decode; neighbours unaffected (above)
    bb = bad.repeat_interleave(256)[:n]
    assert bool(scales[bad].isnan().all()) and not q[bb].any() and not bool(torch.isfinite(dec[bb]).any())


def make_grads(n: int, dtype, steps: int = 3, seed: int = 0, special: bool = False):
    """Seeded randn * 1e-3 gradients; ``special``: block 1 all zero (when there is one), a NaN in
    block 0 and an Inf in the last block at step 1."""
    gen = torch.Generator().manual_seed(seed + n)
    gs = [(torch.randn(n, generator=gen) * 1e-3).to(dtype) for _ in range(steps)]
    if special:
        for g in gs:
            g[256:512] = 0
        gs[1][7] = float("nan")
        gs[1][n - 1] = float("inf")
    return gs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n", [255, 257, 4097])
def test_encode_properties_chained(n, dtype):
    c = Q.Q8Codec(n)
    for g in make_grads(n, dtype):
        acc = c.resid + g.float()
        p = c.encode(g)
        check_step(acc, p, c.resid, n)


def test_zero_and_nonfinite_blocks():
    n = 4097
    c = Q.Q8Codec(n)
    for step, g in enumerate(make_grads(n, torch.float32, special=True)):
        acc = c.resid + g.float()
        p = c.encode(g)
        check_step(acc, p, c.resid, n)
        _, scales, q = Q.views(p, n)
        assert scales[1] == 0 and not q[256:512].any()
        if step >= 1:  # the NaN / Inf blocks stay poisoned through the residual; the others do not
            assert scales[0].isnan() and scales[-1].isnan() and bool(torch.isfinite(scales[1:-1]).all())


def test_subrange_encode_decode_matches_whole():
    n = 4097
    g = make_grads(n, torch.float32, steps=1)[0]
    whole, parts = Q.Q8Codec(n), Q.Q8Codec(n)
    whole.encode(g)
    Q.encode_into(g, parts.resid, parts.payload, n, 0, 2048)
    Q.encode_into(g, parts.resid, parts.payload, n, 2048, n - 2048)
    assert torch.equal(whole.payload, parts.payload) and torch.equal(whole.resid, parts.resid)
    out = torch.full((n,), 3.0)
    Q.decode(whole.payload, n, out=out, scale=0.5, add=True, off=2048, cnt=n - 2048)
    ref = Q.decode(whole.payload, n, out=torch.full((n,), 3.0), scale=0.5, add=True)
    assert torch.equal(out[2048:], ref[2048:]) and bool((out[:2048] == 3.0).all())
    with pytest.raises(ValueError):
        Q.encode_into(g, parts.resid, parts.payload, n, 100, 256)


def _two_servers(codec_cfg, lay, arena, counters):
    out = []
    for _ in range(2):
        s = ParameterServer(codec_cfg, lay, arena.clone(), counters, total_workers=1, log=lambda *a: None)
        s.register_worker("w", 0)
        out.append(s)
    return out


def test_error_feedback_telescopes():
    """T pushes through Q8Codec against the same gradients sent dense: sum_t deq_t =
    sum_t g_t - resid_T, so params_q8 - lr * resid_T must equal params_dense up to the fp32
    rounding of the 2 * T updates and the final correction — each at most half an ulp of the
    parameter, (2 T + 2) / 2 ulps of the largest |p| in all (~1e-6). A lost or double-counted
    residual is off by lr * |resid| ~ 1e-5 (checked below with a doubled residual)."""
    torch.manual_seed(3)
    T, lr = 8, 0.1
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    n = lay.param_numel
    cfg = tiny_cfg(mode="async", workers=1, codec="q8", lr=lr)
    sq, sd = _two_servers(cfg, lay, arena, counters)
    enc = Q.Q8Codec(n)
    gen = torch.Generator().manual_seed(5)
    for _ in range(T):
        g = torch.randn(n, generator=gen) * 1e-2
        for s, wire in ((sq, None), (sd, g)):
            _, gs = s.fetch_parameters(0)
            assert s.push_gradients(0, enc.encode(g) if wire is None else wire, gs)
    assert sq.core.global_step == T and sd.core.global_step == T
    assert sq.bytes_pushed == T * Q.payload_bytes(n)
    atol = (2 * T + 2) / 2 * 2.0 ** -23 * float(sd.params.abs().max())
    assert torch.allclose(sq.params - lr * enc.resid, sd.params, rtol=0, atol=atol)
    assert not torch.allclose(sq.params - 2 * lr * enc.resid, sd.params, rtol=0, atol=atol)


@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_server_q8_apply_matches_dense(mom):
    torch.manual_seed(1)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    n = lay.param_numel
    cfg = tiny_cfg(mode="async", workers=1, codec="q8", momentum=mom)
    s1, s2 = _two_servers(cfg, lay, arena, counters)
    enc = Q.Q8Codec(n)
    for _ in range(2):  # the second push exercises the momentum buffer
        p = enc.encode(torch.randn(n))
        dense = Q.decode(p, n)
        for s, wire in ((s1, p), (s2, dense)):
            _, gs = s.fetch_parameters(0)
            assert s.push_gradients(0, wire, gs)
    assert torch.equal(s1.arena, s2.arena)


@pytest.mark.parametrize("mode,workers", [("sync", 2), ("async", 3)])
def test_run_local_q8(mode, workers):
    cfg = tiny_cfg(mode=mode, workers=workers, codec="q8", eval_every=0)
    res = run_local(cfg, log=lambda *a, **k: None)
    srv = res["server"]
    steps = -(-(96 // workers) // 8)
    assert srv["gradients_processed"] == workers * steps
    fp16_bytes = workers * steps * 2 * ParamLayout.from_module(TinyResNet(10)).param_numel
    assert 0.5 < srv["bytes_pushed"] / fp16_bytes < 0.52


def test_run_local_q8_reference_semantics():
    cfg = tiny_cfg(mode="sync", workers=2, codec="q8", eval_every=0, sync_semantics="reference")
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    assert srv["global_steps_completed"] > 0


@pytest.mark.parametrize("args", [["--mode", "sync"], ["--mode", "sync", "--topology", "dedicated"],
                                  ["--mode", "async", "--staleness-bound", "50"]])
def test_dist_q8_gloo(args):
    recs, _ = _spawn(3, args + ["--codec", "q8"] + TINY)
    srv = [r for r in recs if r["type"] == "SERVER_FINAL_METRICS"][0]
    assert srv["global_steps_completed"] > 0 and srv["gradients_processed"] > 0
    if "sync" in args:  # every round's payloads are counted once, whole
        n = ParamLayout.from_module(TinyResNet(10)).param_numel
        assert srv["bytes_pushed"] == srv["gradients_processed"] * Q.payload_bytes(n)


def test_config_scope():
    with pytest.raises(ValueError):
        PSConfig(codec="q8", topology="sharded").validate()
    with pytest.raises(ValueError):
        PSConfig(codec="q9").validate()
    cfg = PSConfig(mode="sync", codec="q8").validate()
    assert cfg.resolve_overlap(8) is False and not cfg.dense_wire
    assert PSConfig(mode="sync", codec="fp16").validate().resolve_overlap(8) is True
