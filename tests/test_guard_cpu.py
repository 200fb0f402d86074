"""Global-norm clipping and the non-finite guard (--clip-norm, --skip-nonfinite) on the CPU path:
configuration scope, the torch implementation in ParameterServer against
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on fp64 copies, skipped rounds, the encoded
wires, the metrics record, and the guard-off regression. The oracle (GuardOracle) is shared with
the GPU server tests."""
import math
import types

import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel import q8 as Q
from psx.parallel import topk as T
from psx.parallel.server import ParameterServer, arena_sha256
from psx.utils.config import PSConfig, parse

from .test_ps_cpu import tiny_cfg

GUARD_KEYS = {"clip_norm", "rounds", "clipped_rounds", "skipped_rounds", "norm_last", "norm_max", "norm_mean"}


class GuardOracle:
    """torch's own clipping and SGD on an fp64 copy of the trainable prefix. ``step(s, weight)``
    takes the fp32 sum of the round's decoded wires and the round's weight; the gradient torch
    sees is weight * s. ``path`` is |p0| + sum |p_k+1 - p_k|, what each element's value was summed
    from: the tolerance of the comparisons is relative to it (tests/test_dcasgd_gpu.py)."""

    def __init__(self, p0, lr, momentum, wd, clip_norm):
        self.p = torch.nn.Parameter(p0.detach().double().clone())
        self.opt = torch.optim.SGD([self.p], lr=lr, momentum=momentum, weight_decay=wd)
        self.clip_norm = clip_norm
        self.path = self.p.detach().abs().clone()
        self.norms = []

    def step(self, s, weight):
        before = self.p.detach().clone()
        self.p.grad = float(weight) * s.double()
        norm = float(self.p.grad.norm())
        self.norms.append(norm)
        if self.clip_norm > 0:
            torch.nn.utils.clip_grad_norm_([self.p], self.clip_norm)
        self.opt.step()
        self.path += (self.p.detach() - before).abs()
        return norm


def assert_path_close(got, oracle: GuardOracle, what=""):
    diff = (got.double().cpu() - oracle.p.detach()).abs()
    bad = diff > 1e-5 * oracle.path
    assert not bool(bad.any()), (what, int(bad.sum()), float((diff / oracle.path.clamp_min(1e-300)).max()))


def fp32_sum(wires):
    """The fp32 sum of dense wires in source order, starting from 0.f."""
    s = torch.zeros(wires[0].numel(), dtype=torch.float32)
    for w in wires:
        s += w.float().cpu()
    return s


def tiny_server(mode="sync", workers=3, device="cpu", **kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(mode=mode, workers=workers, **kw)
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=workers, log=lambda *a: None)
    for w in range(workers):
        s.register_worker(f"w{w}", w)
    return s, lay, cfg


# rounds 0, 2, 4 are small and 1, 3, 5 sixteen times larger: a bound between the two groups clips three
SCALES = [0.01, 0.16, 0.01, 0.16, 0.01, 0.16]


def round_wires(n, workers, dtype=torch.float16, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return [[(torch.randn(n, generator=gen) * sc).to(dtype) for _ in range(workers)] for sc in SCALES]


def clip_between(rounds, weight):
    """A bound between the small and the large rounds' norms (geometric middle)."""
    norms = sorted(weight * float(fp32_sum(ws).double().norm()) for ws in rounds)
    assert norms[2] * 4 < norms[3]
    return math.sqrt(norms[2] * norms[3])


# ---------------------------------------------------------------------------- configuration
def test_config_scope():
    d = PSConfig().validate()
    assert d.clip_norm == 0.0 and d.skip_nonfinite is False and d.grad_guard is False
    c = PSConfig(clip_norm=1.0).validate()
    assert c.skip_nonfinite is True and c.grad_guard is True
    assert PSConfig(skip_nonfinite=True).validate().grad_guard is True
    with pytest.raises(ValueError, match="--clip-norm"):
        PSConfig(clip_norm=-1.0).validate()
    for on in (dict(clip_norm=1.0), dict(skip_nonfinite=True)):
        for bad in (dict(optimizer="lars"), dict(mode="async", dc_lambda=0.04), dict(topology="sharded"),
                    dict(overlap=True)):
            with pytest.raises(ValueError, match="--clip-norm"):
                PSConfig(**on, **bad).validate()
        assert PSConfig(mode="sync", **on).validate().resolve_overlap(4) is False
        assert PSConfig(mode="sync", overlap=False, **on).validate().resolve_overlap(4) is False
    assert PSConfig(mode="sync").validate().resolve_overlap(4) is True


def test_cli_flags_and_checkpoint_config():
    import json

    cfg = parse(["--clip-norm", "0.5"])
    assert cfg.clip_norm == 0.5 and cfg.skip_nonfinite is True
    assert parse(["--skip-nonfinite"]).grad_guard and parse(["--skip-nonfinite"]).clip_norm == 0.0
    assert not parse([]).grad_guard
    with pytest.raises(ValueError):
        parse(["--clip-norm", "-2"])
    saved = json.loads(cfg.to_json())  # what a checkpoint carries
    assert saved["clip_norm"] == 0.5 and saved["skip_nonfinite"] is True


def test_native_paths_decline_the_guard(monkeypatch):
    """Per-bucket and native async paths fall back to the Python server (or refuse) with the
    guard on; the native sync serial round keeps serving it."""
    from psx.parallel.graph_round import graph_round_enabled
    from psx.parallel.native_loop import NativeServerLoop, native_loop_enabled
    from psx.parallel.native_sync import native_sync_enabled
    from psx.parallel.runner import run_local_threads
    from psx.parallel.worker import SyncCollectiveChannel

    for k in ("PSX_NATIVE_LOOP", "PSX_NATIVE_SYNC", "PSX_SYNC_AGG"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PSX_GRAPH_ROUND", "1")
    t = types.SimpleNamespace(native=True, world_size=3, rank=0)
    srv = types.SimpleNamespace(wire=None)
    for clip, want in ((0.0, True), (1.0, False)):
        assert native_loop_enabled(PSConfig(mode="async", clip_norm=clip).validate(), t) is want
        assert graph_round_enabled(PSConfig(mode="sync", topology="colocated", clip_norm=clip).validate(), t) is want
        s = PSConfig(mode="sync", topology="dedicated", clip_norm=clip).validate()
        chan = SyncCollectiveChannel(t, srv, members=[0, 1], codec=None, root_worker=False)
        assert native_sync_enabled(s, t, chan, srv, 0) is True
    on = PSConfig(mode="async", skip_nonfinite=True).validate()
    stub = types.SimpleNamespace(cfg=on, layout=None, device="cpu")
    with pytest.raises(ValueError, match="--clip-norm"):
        NativeServerLoop(stub, None, None, {}, 1)
    with pytest.raises(ValueError, match="--clip-norm"):
        run_local_threads(on, 1)


# ---------------------------------------------------------------------------- server numerics
@pytest.mark.parametrize("mode", ["sync", "async"])
def test_cpu_arena_matches_torch_clipping(mode):
    """push_gradients on a CPU arena, 6 rounds of fp16 wires, momentum 0.9, weight decay 5e-4,
    against clip_grad_norm_ + SGD in fp64 fed the same decoded sums; three rounds clip, three do
    not."""
    W = 3 if mode == "sync" else 1
    hp = dict(codec="fp16", momentum=0.9, weight_decay=5e-4, lr=0.05)
    probe, lay, _ = tiny_server(mode, W, **hp)
    rounds = round_wires(lay.param_numel, W)
    C = clip_between(rounds, 1.0 / W)
    s, lay, cfg = tiny_server(mode, W, clip_norm=C, **hp)
    oracle = GuardOracle(s.params, cfg.lr, cfg.momentum, cfg.weight_decay, C)
    for k, wires in enumerate(rounds):
        for w, g in enumerate(wires):
            assert s.push_gradients(w, g, s.core.global_step)
        norm = oracle.step(fp32_sum(wires), s.last_push.weight)
        assert s.core.global_step == k + 1
        assert_path_close(s.params, oracle, (mode, k))
        assert s.guard_counters()["norm_last"] == pytest.approx(norm, rel=1e-6)
    g = s.final_metrics()["gradient_guard"]
    assert (g["rounds"], g["clipped_rounds"], g["skipped_rounds"]) == (6, 3, 0)
    assert sum(nm > C for nm in oracle.norms) == 3
    assert g["norm_max"] == pytest.approx(max(oracle.norms), rel=1e-6)
    assert g["norm_mean"] == pytest.approx(sum(oracle.norms) / 6, rel=1e-6)
    # the clipping is far above the tolerance: the same rounds without it end somewhere else
    for wires in rounds:
        for w, g_ in enumerate(wires):
            probe.push_gradients(w, g_, probe.core.global_step)
    assert not torch.allclose(probe.params, s.params, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("bad_round", [0, 1])
@pytest.mark.parametrize("where,value", [("first", float("inf")), ("last", float("-inf")), ("mid", float("nan"))])
def test_nonfinite_round_is_skipped(where, value, bad_round):
    """One worker's wire holds inf / NaN: arena and momentum buffer bit-unchanged, the round
    counted; the next finite round equals a run that never saw the bad one (also when the bad
    round was the first and consumed the momentum first-step flag)."""
    W = 3
    hp = dict(codec="fp16", momentum=0.9, weight_decay=5e-4, lr=0.05, skip_nonfinite=True)
    s, lay, cfg = tiny_server("sync", W, **hp)
    r, _, _ = tiny_server("sync", W, **hp)  # never sees the bad round
    n = lay.param_numel
    good = round_wires(n, W)[:2]
    oracle = GuardOracle(s.params, cfg.lr, cfg.momentum, cfg.weight_decay, 0.0)
    bad = [g.clone() for g in good[0]]
    bad[1][{"first": 0, "last": n - 1, "mid": n // 2}[where]] = value
    seq = [good[0], good[1]]
    seq.insert(bad_round, None)
    for wires in seq:
        if wires is None:
            before, step = (s.arena.clone(), s.momentum_buf.clone()), s.core.global_step
            for w, g in enumerate(bad):
                s.push_gradients(w, g, step)
            assert torch.equal(s.arena, before[0]) and torch.equal(s.momentum_buf, before[1])
            assert s.core.global_step == step + 1
            c = s.guard_counters()
            assert c["skipped_rounds"] == 1 and not math.isfinite(c["norm_last"])
            continue
        for w, g in enumerate(wires):
            s.push_gradients(w, g, s.core.global_step)
            r.push_gradients(w, g, r.core.global_step)
        oracle.step(fp32_sum(wires), 1.0 / W)
        assert torch.equal(s.arena, r.arena) and torch.equal(s.momentum_buf, r.momentum_buf)
        assert_path_close(s.params, oracle, (where, bad_round))
    g = s.final_metrics()["gradient_guard"]
    assert (g["rounds"], g["clipped_rounds"], g["skipped_rounds"]) == (3, 0, 1)
    assert math.isfinite(g["norm_max"]) and math.isfinite(g["norm_mean"])
    assert r.final_metrics()["gradient_guard"]["rounds"] == 2
    assert bool(torch.isfinite(s.arena).all())


def test_without_the_guard_the_same_wire_poisons_the_arena():
    s, lay, _ = tiny_server("async", 1, codec="fp16")
    g = torch.zeros(lay.param_numel, dtype=torch.float16)
    g[0] = float("inf")
    s.push_gradients(0, g, 0)
    assert not bool(torch.isfinite(s.arena).all())


@pytest.mark.parametrize("kind", ["q8", "topk"])
def test_encoded_wires_take_the_dense_path(kind):
    """q8 / top-k payloads are decoded into the aggregation buffer and clipped there: against the
    oracle fed the decoded gradient (no direct scatter, even without momentum and weight decay)."""
    hp = dict(codec=kind, lr=0.05, topk_ratio=0.25)
    n = tiny_server("async", 1, **hp)[1].param_numel
    # dense norms about 0.001 sqrt(n) and 0.05 sqrt(n) (top-k keeps the largest quarter: somewhat
    # less); the bound lies a factor 7 from either
    C = 0.007 * math.sqrt(n)
    s, lay, cfg = tiny_server("async", 1, clip_norm=C, **hp)
    oracle = GuardOracle(s.params, cfg.lr, 0.0, 0.0, C)
    gen = torch.Generator().manual_seed(11)
    enc = Q.Q8Codec(n) if kind == "q8" else T.TopKCodec(n, cfg.topk_ratio, "cpu")
    for k, sc in enumerate((0.001, 0.05)):
        enc.resid.zero_()
        wire = enc.encode(torch.randn(n, generator=gen) * sc).clone()
        dense = Q.decode(wire, n) if kind == "q8" else \
            T.decode_add(wire, torch.zeros(n), 1.0, T.topk_k(n, cfg.topk_ratio)).clone()
        assert s.push_gradients(0, wire, k)
        oracle.step(dense, s.last_push.weight)
        assert_path_close(s.params, oracle, (kind, k))
    g = s.guard_counters()
    assert (g["rounds"], g["clipped_rounds"], g["skipped_rounds"]) == (2, 1, 0)


def test_partial_range_raises():
    s, lay, _ = tiny_server("sync", 1, codec="none", clip_norm=1.0)
    n = lay.param_numel
    g = torch.zeros(n)
    with pytest.raises(ValueError, match="--clip-norm"):
        s.apply_range(g[: n // 2], 1.0, 0, n // 2)
    with pytest.raises(ValueError, match="--clip-norm"):
        s.apply_range_sources([g], 1.0, 8, n)


# ---------------------------------------------------------------------------- metrics
def test_metrics_record():
    off, lay, _ = tiny_server("async", 1)
    assert "gradient_guard" not in off.final_metrics() and off.guard_counters() is None
    lines = []
    cfg = tiny_cfg(mode="async", workers=1, codec="none", clip_norm=2.0, verbose=1)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    on = ParameterServer(cfg, lay, arena, counters, total_workers=1, log=lambda *a, **k: lines.append(a[0]))
    g = on.final_metrics()["gradient_guard"]
    assert set(g) == GUARD_KEYS and g["rounds"] == 0 and g["norm_mean"] is None and g["clip_norm"] == 2.0
    on.register_worker("w", 0)
    bad = torch.zeros(lay.param_numel)
    bad[3] = float("nan")
    on.push_gradients(0, bad, 0)
    on.push_gradients(0, torch.full((lay.param_numel,), 1e-3), 1)
    assert not any("GradientGuard" in ln for ln in lines)  # not per round: at the metrics read
    g = on.final_metrics()["gradient_guard"]
    on.final_metrics()
    assert sum("GradientGuard" in ln for ln in lines) == 1  # once
    assert set(g) == GUARD_KEYS and (g["rounds"], g["clipped_rounds"], g["skipped_rounds"]) == (2, 0, 1)
    assert g["norm_mean"] == pytest.approx(1e-3 * math.sqrt(lay.param_numel), rel=1e-5) == g["norm_max"]


def test_run_local_sync_with_clipping():
    from psx.parallel.runner import run_local

    cfg = tiny_cfg(mode="sync", workers=2, clip_norm=0.05, momentum=0.9, eval_every=0)
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    g = srv["gradient_guard"]
    assert srv["global_steps_completed"] > 0 and g["rounds"] == srv["global_steps_completed"]
    assert g["clipped_rounds"] > 0 and g["skipped_rounds"] == 0 and math.isfinite(srv["final_param_checksum"])


# ---------------------------------------------------------------------------- guard off: nothing changes
def test_guard_off_keeps_the_sgd_bits():
    """Three sync rounds with the guard off end in the bits of the SGD update written out here
    (the CPU arena's formula of apply_range): the guard's routing does not touch the default."""
    W = 3
    s, lay, cfg = tiny_server("sync", W, codec="fp16", momentum=0.9, weight_decay=5e-4, lr=0.05)
    assert s._guard is False and s.agg is None
    arena = s.arena.clone()
    p = arena[: lay.param_numel]
    buf = torch.zeros_like(p)
    for k, wires in enumerate(round_wires(lay.param_numel, W)[:3]):
        for w, g in enumerate(wires):
            s.push_gradients(w, g, s.core.global_step)
        agg = wires[0].float()
        for g in wires[1:]:
            agg.add_(g.float())
        d = agg * s.last_push.weight + cfg.weight_decay * p
        if k == 0:
            buf.copy_(d)
        else:
            buf.mul_(cfg.momentum).add_(d)
        p.sub_(cfg.lr * buf)
    assert s.final_metrics()["final_param_sha256"] == arena_sha256(arena)
