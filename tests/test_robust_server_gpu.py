"""--aggregate trimmed / median / krum in the device ParameterServer: W = 5 gathered fp16 wires
through apply_sources against the CPU-arena server (combine_host, then the rule's host form), one
wildly wrong worker against the honest wires' spread, and the metrics."""
import pytest
import torch

from psx.parallel.runner import build_state
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

pytestmark = pytest.mark.gpu

W, LR = 5, 0.05
OPTS = {"sgd": dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4), "adamw": dict(optimizer="adamw", lr=1e-3)}


def _server(device, **kw):
    kw = {"lr": LR, **kw}
    cfg = PSConfig(model="resnet_tiny", workers=W, eval_every=0, verbose=0, heartbeat_timeout=0, **kw).validate()
    _, lay, arena, counters = build_state(cfg)
    srv = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=W, log=lambda *a, **k: None)
    for w in range(W):
        srv.register_worker(f"w{w}", w)
    return srv


@pytest.fixture(scope="module")
def rounds():
    """Two rounds of W fp16 wires: a common direction plus noise; worker 3 is 1e4 times too large."""
    n = _server("cpu").n
    gen = torch.Generator().manual_seed(11)
    out = []
    for _ in range(2):
        base = torch.randn(n, generator=gen) * 1e-2
        row = [(base + torch.randn(n, generator=gen) * 1e-3).half() for _ in range(W)]
        row[3] = (row[3].float() * 1e4).half()
        out.append(row)
    return out


def _drive(srv, rounds):
    """apply_sources round by round; returns |p0| + sum |p_k+1 - p_k|."""
    path = srv.params.abs().double()
    for row in rounds:
        before = srv.params.clone()
        gs = srv.core.global_step
        assert srv.apply_sources([g.to(srv.device) for g in row], list(range(W)), [gs] * W)
        path += (srv.params.double() - before.double()).abs()
    return path.cpu()


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("agg", ["trimmed", "median", "krum"])
def test_device_server_matches_cpu_arena(agg, opt, rounds):
    cpu, dev = _server("cpu", aggregate=agg, **OPTS[opt]), _server("cuda", aggregate=agg, **OPTS[opt])
    _drive(cpu, rounds)
    path = _drive(dev, rounds)
    torch.cuda.synchronize()
    # rtol 1e-5 relative to each element's start plus the steps it took (tests/test_guard_server_gpu.py)
    diff = (cpu.params.double() - dev.params.double().cpu()).abs()
    print(f"{agg} {opt}: max |diff| / path {(diff / path.clamp_min(1e-300)).max().item():.3e}")
    assert bool((diff <= 1e-5 * path).all())
    m = dev.final_metrics()["robust_aggregate"]
    assert (m["kind"], m["rounds"]) == (agg, 2) and m == cpu.final_metrics()["robust_aggregate"]
    if agg == "krum":
        assert m["krum_selected_per_worker"] == [2, 2, 2, 0, 2]


def test_one_wrong_worker_moves_the_mean_but_not_the_trimmed_mean(rounds):
    row = rounds[0]
    honest = torch.stack([g.float() for k, g in enumerate(row) if k != 3])
    lo, hi = LR * honest.min(0).values.double(), LR * honest.max(0).values.double()
    step = {}
    for agg in ("trimmed", "mean"):
        srv = _server("cuda", aggregate=agg, optimizer="sgd", momentum=0.9)
        p0 = srv.params.clone()
        _drive(srv, [row])
        step[agg] = (p0.double() - srv.params.double()).cpu()  # lr * the estimate: first momentum step, no decay
    tol = 2.0 ** -22 * (_server("cpu").params.abs().double() + hi.abs() + lo.abs())  # the fp32 update's rounding
    assert bool(((step["trimmed"] >= lo - tol) & (step["trimmed"] <= hi + tol)).all())
    assert not bool(((step["mean"] >= lo - tol) & (step["mean"] <= hi + tol)).all())
