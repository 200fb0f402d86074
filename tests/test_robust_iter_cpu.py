"""--aggregate geomed / cclip on the CPU: combine_host (parallel/robust.py) against a numpy fp64
implementation of the module docstring's definitions, robustness on a contaminated round, the
refusals of PSConfig.validate and the CPU server."""
import numpy as np
import pytest
import torch

from psx.parallel import robust as RB
from psx.parallel.runner import build_state
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig, parse

U = 2.0 ** -24


def ref64(x, kind, L, tau=0.0, nu=1e-6, v=None):
    """geomed / cclip on x [W, n] in fp64 from the centre v (None: zeros): (v_L, a, d)."""
    W, n = x.shape
    v = np.zeros(n) if v is None else v
    for _ in range(L):
        d2 = ((x - v) ** 2).sum(1)
        d = np.sqrt(np.where(np.isfinite(d2), d2, np.inf))
        with np.errstate(divide="ignore"):
            if kind == "geomed":
                w = np.where(np.isinf(d), 0.0, 1.0 / np.maximum(d, nu))
                a, b = w / w.sum() if w.sum() > 0 else w, 0.0
            else:
                a = np.where(np.isinf(d), 0.0, np.minimum(1.0, tau / d)) / W
                b = 1.0 - a.sum()
        v = b * v + sum(a[k] * x[k] for k in range(W) if a[k] != 0.0)
    return v, a, d


def contaminated():
    """n = 20005: five honest fp16 wires mu + noise (both N(0, 1e-2^2), seed 0), one wire -1e3 mu, one
    all NaN. Returns (wires [7, n] fp16, the honest mean in fp64, r = the largest distance of an honest
    wire from it)."""
    gen, n = torch.Generator().manual_seed(0), 20005
    mu = torch.randn(n, generator=gen) * 1e-2
    x = torch.stack([mu + torch.randn(n, generator=gen) * 1e-2 for _ in range(5)] + [-1e3 * mu, mu * float("nan")])
    x = x.half()
    h = x[:5].double().numpy()
    return x, h.mean(0), np.sqrt(((h - h.mean(0)) ** 2).sum(1)).max()


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("W", [3, 4, 7, 8, 32])
@pytest.mark.parametrize("kind", ["geomed", "cclip"])
def test_combine_host_against_fp64(kind, W, L):
    n = 1000
    x = (torch.randn(W, n, generator=torch.Generator().manual_seed(W)) * 0.1 + 0.05).half()
    x[0] *= 30.0  # one wire far out: clipped by cclip, down-weighted by geomed
    v0 = torch.full((n,), 0.04)
    tau = 3.0  # the honest wires are about 0.1 * sqrt(n) = 3.2 from the centre: both sides of the clip
    got, (a, d) = RB.combine_host(list(x), n, kind, iters=L, tau=tau, centre=v0.clone())
    want, a64, d64 = ref64(x.double().numpy(), kind, L, tau, v=v0.double().numpy() if kind == "cclip" else None)
    assert np.abs(a - a64).max() <= 1e-5 * a64.max() and np.abs(d - d64).max() <= 1e-5 * d64.max()
    # every step's fp32 chain of W + 1 terms is within (W + 1) u of the sum of its terms' magnitudes, and the
    # weights move with the distances by a relative 1e-5 at most (asserted above): 1e-4 of that sum covers L steps
    mag = np.abs(x.double().numpy()).T @ a64 + (0.04 if kind == "cclip" else 0.0) + np.abs(want)
    assert (np.abs(got.double().numpy() - want) <= 1e-4 * mag).all()


@pytest.mark.parametrize("kind", ["geomed", "cclip"])
def test_contaminated_round_stays_within_the_honest_spread(kind):
    x, honest, r = contaminated()
    centre = torch.zeros(x.shape[1])
    for rnd in range(3 if kind == "cclip" else 1):
        e, (a, _) = RB.combine_host(list(x), x.shape[1], kind, iters=3, tau=1.0, centre=centre)
        dist = np.sqrt(((e.double().numpy() - honest) ** 2).sum())
        print(f"{kind} round {rnd + 1}: {dist / r:.3f} r, a = {a}")
        assert dist <= r and a[6] == 0.0 and a[5] < 1e-3 and bool(torch.isfinite(e).all())


@pytest.mark.parametrize("argv,fragment", [
    (["--codec", "q8"], "fp16 or none only"),
    (["--codec", "powersgd"], "fp16 or none only"),
    (["--mode", "async"], "--mode sync only"),
    (["--mode", "async", "--dc-lambda", "0.1"], "not with --dc-lambda"),
    (["--topology", "sharded"], "not with --topology sharded"),
    (["--overlap"], "not with --overlap"),
    (["--trim", "0"], "must be >= 1"),
    (["--robust-iters", "0"], "--robust-iters must be >= 1"),
    (["--geomed-eps", "0"], "--geomed-eps must be > 0"),
])
@pytest.mark.parametrize("kind", [["geomed"], ["cclip", "--cclip-tau", "1.0"]])
def test_validate_refuses(kind, argv, fragment):
    with pytest.raises(ValueError, match=fragment):
        parse(["--aggregate"] + kind + argv)


def test_validate_cclip_needs_tau_and_no_overlap(monkeypatch):
    with pytest.raises(ValueError, match="--cclip-tau > 0"):
        parse(["--aggregate", "cclip"])
    monkeypatch.setenv("PSX_SYNC_AGG", "reduce")
    with pytest.raises(ValueError, match="PSX_SYNC_AGG=reduce"):
        parse(["--aggregate", "geomed"])
    monkeypatch.delenv("PSX_SYNC_AGG")
    assert not parse(["--aggregate", "geomed"]).resolve_overlap(4)
    assert not parse(["--aggregate", "cclip", "--cclip-tau", "2"]).resolve_overlap(4)


def _server(W, **kw):
    cfg = PSConfig(model="resnet_tiny", workers=W, lr=0.05, eval_every=0, verbose=0, heartbeat_timeout=0,
                   **kw).validate()
    _, lay, arena, counters = build_state(cfg)
    srv = ParameterServer(cfg, lay, arena.clone(), counters, device="cpu", total_workers=W, log=lambda *a, **k: None)
    for w in range(W):
        srv.register_worker(f"w{w}", w)
    return srv


@pytest.mark.parametrize("kw", [dict(aggregate="geomed"), dict(aggregate="cclip", cclip_tau=1.0)])
def test_short_round_and_partial_range_are_refused(kw):
    srv = _server(2, **kw)
    wires = [torch.zeros(srv.n, dtype=torch.float16) for _ in range(2)]
    with pytest.raises(ValueError, match="at least 3 sources, this round has 2"):
        srv.update_range(wires, 0.5, 0, srv.n)
    srv, before = _server(3, **kw), None
    before = srv.params.clone()
    with pytest.raises(ValueError, match="scores the workers over the whole gradient"):
        srv.update_range([torch.ones(8, dtype=torch.float16) for _ in range(3)], 1.0 / 3, 0, 8)
    assert torch.equal(srv.params, before)


def test_geomed_round_ignores_a_scaled_and_a_nan_worker():
    # the geometric median of {g, g, g, 1e4 g} is g, and Weiszfeld from 0 closes in on it linearly: v_L = (1 + 3^-L) g, every
    # step cutting the excess to a third (--robust-iters 16 here). lr |g|_max 3^-L <= 0.05 * 6 * 3^-16 = 7e-9 leaves atol to the fp32 weights (3 u lr |g|_max = 5e-8)
    srv, ref = _server(5, aggregate="geomed", robust_iters=16), _server(5)
    g = torch.randn(srv.n, generator=torch.Generator().manual_seed(2)).half()
    for w, wire in enumerate([g, g, g, 1e4 * g, g * float("nan")]):
        srv.push_gradients(w, wire.clone(), 0)
    for w in range(5):
        ref.push_gradients(w, g.clone(), 0)
    assert torch.allclose(srv.params, ref.params, rtol=0, atol=1e-6)
    m = srv.final_metrics()["robust_aggregate"]
    assert set(m) == {"kind", "rounds", "iters", "degenerate_rounds", "geomed_mean_weight_per_worker"}
    assert (m["kind"], m["rounds"], m["iters"], m["degenerate_rounds"]) == ("geomed", 1, 16, 0)
    assert m["geomed_mean_weight_per_worker"][4] == 0.0 and len(m["geomed_mean_weight_per_worker"]) == 5
    c = _server(3, aggregate="cclip", cclip_tau=1.0).final_metrics()["robust_aggregate"]
    assert c == {"kind": "cclip", "rounds": 0, "iters": 3, "degenerate_rounds": 0, "tau": 1.0,
                 "cclip_clipped_per_worker": [0, 0, 0]}
