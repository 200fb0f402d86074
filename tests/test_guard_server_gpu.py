"""The gradient guard (--clip-norm, --skip-nonfinite) in the device ParameterServer: loopback
pushes of every wire kind against the CPU-arena server (itself checked against torch in
tests/test_guard_cpu.py), the gathered multi-source entry against the loopback's dense entry, and
whole loopback runs with the guard off, idle and clipping."""
import pytest
import torch

from psx.parallel import q8 as Q
from psx.parallel import topk as T
from psx.parallel.runner import build_state, run_local
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

pytestmark = pytest.mark.gpu

SCALES = [0.01, 0.04, 0.01, 0.04]  # the bound is twice the first round's norm: rounds 1 and 3 clip
TOPK_RATIO = 0.25


def _server(device, mode, W, codec, **kw):
    cfg = PSConfig(model="resnet_tiny", mode=mode, workers=W, lr=0.05, staleness_bound=50, codec=codec, momentum=0.9,
                   weight_decay=5e-4, eval_every=0, verbose=0, heartbeat_timeout=0, topk_ratio=TOPK_RATIO,
                   **kw).validate()
    _, lay, arena, counters = build_state(cfg)
    srv = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=W, log=lambda *a, **k: None)
    for w in range(W):
        srv.register_worker(f"w{w}", w)
    return srv


def _payloads(n, W, codec):
    """Per round and worker the wire of ``codec``, built on the CPU (every element well away from
    the fp16 underflow, so no wire carries a signed zero)."""
    gen = torch.Generator().manual_seed(9)
    enc = Q.Q8Codec(n) if codec == "q8" else T.TopKCodec(n, TOPK_RATIO, "cpu") if codec == "topk" else None
    out = []
    for sc in SCALES:
        row = []
        for _ in range(W):
            g = torch.randn(n, generator=gen)
            g = torch.where(g >= 0, 1.0, -1.0) * (g.abs() * sc + 1e-4)
            if enc is not None:
                enc.resid.zero_()
                row.append(enc.encode(g).clone())
            else:
                row.append(g.half() if codec == "fp16" else g)
        out.append(row)
    return out


def _drive(srv, rounds):
    """push_gradients round by round; returns |p0| + sum |p_k+1 - p_k| over the applies."""
    path = srv.params.abs().double()
    for row in rounds:
        for w, g in enumerate(row):
            before = srv.params.clone()
            srv.push_gradients(w, g.to(srv.device), srv.core.global_step)
            path += (srv.params.double() - before.double()).abs()
    return path.cpu()


@pytest.mark.parametrize("codec", ["fp16", "none", "q8", "topk"])
@pytest.mark.parametrize("mode,W", [("sync", 1), ("sync", 3), ("async", 1), ("async", 3)])
def test_device_server_matches_cpu_arena(mode, W, codec):
    probe = _server("cpu", mode, W, codec, skip_nonfinite=True)
    rounds = _payloads(probe.n, W, codec)
    _drive(probe, rounds[:1])
    C = 2.0 * probe.guard_counters()["norm_max"]  # from the first round's norm (async: its largest push)
    cpu, dev = _server("cpu", mode, W, codec, clip_norm=C), _server("cuda", mode, W, codec, clip_norm=C)
    dev.enable_weight_wire()
    _drive(cpu, rounds)
    path = _drive(dev, rounds)
    torch.cuda.synchronize()
    gc, gd = cpu.guard_counters(), dev.guard_counters()
    updates = len(SCALES) * (W if mode == "async" else 1)
    assert gd["rounds"] == gc["rounds"] == updates == dev.core.global_step
    assert gd["clipped_rounds"] == gc["clipped_rounds"] == updates // 2 and gd["skipped_rounds"] == 0
    for k in ("norm_last", "norm_max", "norm_mean"):
        assert gd[k] == pytest.approx(gc[k], rel=1e-5), k
    # rtol 1e-5 relative to each element's start plus the steps it took (tests/test_dcasgd_gpu.py)
    diff = (cpu.params.double() - dev.params.double().cpu()).abs()
    print(f"{mode} W={W} {codec}: max |diff| / path {(diff / path.clamp_min(1e-300)).max().item():.3e}")
    assert bool((diff <= 1e-5 * path).all())
    assert not dev._wire_stale  # the image came out of guard_apply
    assert torch.equal(dev.wire.img[: dev.n].view(torch.int16), dev.params.bfloat16().view(torch.int16))


@pytest.mark.parametrize("codec", ["fp16", "none"])
def test_gathered_and_loopback_rounds_give_the_same_bits(codec):
    """apply_sources (the W wires through the multi-source entry) and the loopback (the wires
    summed into the aggregation buffer by chained fp32 adds, then the dense entry)."""
    W = 3
    probe = _server("cpu", "sync", W, codec, skip_nonfinite=True)
    rounds = _payloads(probe.n, W, codec)
    _drive(probe, rounds[:1])
    C = 2.0 * probe.guard_counters()["norm_max"]
    gathered, loop = _server("cuda", "sync", W, codec, clip_norm=C), _server("cuda", "sync", W, codec, clip_norm=C)
    _drive(loop, rounds)
    for row in rounds:
        gs = gathered.core.global_step
        assert gathered.apply_sources([g.cuda() for g in row], list(range(W)), [gs] * W)
    torch.cuda.synchronize()
    assert torch.equal(gathered.arena, loop.arena) and torch.equal(gathered.momentum_buf, loop.momentum_buf)
    assert gathered.final_metrics()["final_param_sha256"] == loop.final_metrics()["final_param_sha256"]
    a, b = gathered._guard_state.read(), loop._guard_state.read()
    assert a == b and (a["rounds"], a["clipped_rounds"], a["skipped_rounds"]) == (4, 2, 0)


def test_device_server_skips_a_nonfinite_round():
    srv = _server("cuda", "sync", 2, "fp16", skip_nonfinite=True)
    srv.enable_weight_wire()
    rounds = _payloads(srv.n, 2, "fp16")
    _drive(srv, rounds[:1])
    before = (srv.arena.clone(), srv.momentum_buf.clone(), srv.wire.img.clone())
    bad = [g.clone() for g in rounds[1]]
    bad[1][srv.n - 1] = float("inf")  # what the fp16 cast makes of a gradient above 65504
    _drive(srv, [bad])
    torch.cuda.synchronize()
    assert torch.equal(srv.arena, before[0]) and torch.equal(srv.momentum_buf, before[1])
    assert torch.equal(srv.wire.img.view(torch.int16), before[2].view(torch.int16))
    g = srv.final_metrics()["gradient_guard"]
    assert srv.core.global_step == 2 and (g["rounds"], g["skipped_rounds"]) == (2, 1)
    _drive(srv, rounds[2:3])
    assert bool(torch.isfinite(srv.arena).all()) and not torch.equal(srv.arena, before[0])


def _loopback(**kw):
    # the HIP engine's model (resnet_tiny is the CPU suite's torch model: its widths are not the engine's)
    cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.1,
                   max_steps=4, mode="sync", workers=2, deterministic=True, **kw).validate()
    return run_local(cfg, log=lambda *a, **k: None)["server"]


def test_run_local_idle_guard_keeps_the_bits_and_a_tight_bound_clips_every_round():
    off, idle, tight = _loopback(), _loopback(clip_norm=1e9), _loopback(clip_norm=0.05)
    assert off["global_steps_completed"] == idle["global_steps_completed"] == tight["global_steps_completed"] == 4
    assert "gradient_guard" not in off
    assert idle["final_param_sha256"] == off["final_param_sha256"]
    assert (idle["gradient_guard"]["rounds"], idle["gradient_guard"]["clipped_rounds"]) == (4, 0)
    assert tight["final_param_sha256"] != off["final_param_sha256"]
    assert tight["gradient_guard"]["clipped_rounds"] == 4 and tight["gradient_guard"]["skipped_rounds"] == 0
