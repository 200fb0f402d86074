"""--aggregate trimmed / median / krum on the CPU: combine_host (parallel/robust.py) against numpy
fp64, every refusal of PSConfig.validate, the minimum-W error of a short round, and --aggregate mean
leaving update_range's sources alone."""
import numpy as np
import pytest
import torch

from psx.parallel import robust as RB
from psx.parallel.runner import build_state
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig, parse

N = 1000


@pytest.mark.parametrize("kind,T,W", [(k, T, W) for k, T in (("trimmed", 1), ("trimmed", 2), ("median", 0))
                                      for W in (3, 4, 5, 8, 9, 16, 17, 32) if k == "median" or W > 2 * T])
def test_combine_host_against_fp64(kind, T, W):
    x = torch.randn(W, N, generator=torch.Generator().manual_seed(W)).half()
    x[:, ::10] = x[:2, ::10].repeat(W, 1)[:W]  # ties
    got, _ = RB.combine_host(list(x), N, kind, trim=T)
    s = np.sort(x.double().numpy(), axis=0)
    want = np.median(s, axis=0) if kind == "median" else s[T:W - T].mean(axis=0)
    bound = 0.0 if kind == "median" else (W - 2 * T) * 2.0 ** -24 * np.abs(s[T:W - T]).sum(axis=0)
    assert (np.abs(got.double().numpy() - want) <= bound).all()


@pytest.mark.parametrize("argv,fragment", [
    (["--codec", "q8"], "fp16 or none only"),
    (["--codec", "powersgd"], "fp16 or none only"),
    (["--mode", "async"], "--mode sync only"),
    (["--mode", "async", "--dc-lambda", "0.1"], "not with --dc-lambda"),
    (["--topology", "sharded"], "not with --topology sharded"),
    (["--overlap"], "not with --overlap"),
    (["--trim", "0"], "must be >= 1"),
])
@pytest.mark.parametrize("kind", ["trimmed", "median", "krum"])
def test_validate_refuses(kind, argv, fragment):
    with pytest.raises(ValueError, match=fragment):
        parse(["--aggregate", kind] + argv)


def test_validate_refuses_a_reducing_gather(monkeypatch):
    monkeypatch.setenv("PSX_SYNC_AGG", "reduce")
    with pytest.raises(ValueError, match="PSX_SYNC_AGG=reduce"):
        parse(["--aggregate", "median"])
    assert parse([]).aggregate == "mean" and parse([]).resolve_overlap(4)
    monkeypatch.delenv("PSX_SYNC_AGG")
    assert not parse(["--aggregate", "median"]).resolve_overlap(4)


def _server(W, **kw):
    cfg = PSConfig(model="resnet_tiny", workers=W, lr=0.05, eval_every=0, verbose=0, heartbeat_timeout=0,
                   **kw).validate()
    _, lay, arena, counters = build_state(cfg)
    return ParameterServer(cfg, lay, arena.clone(), counters, device="cpu", total_workers=W, log=lambda *a, **k: None)


@pytest.mark.parametrize("kw,W,need", [(dict(aggregate="trimmed", trim=2), 4, 5), (dict(aggregate="krum"), 4, 5)])
def test_a_short_round_raises_with_the_numbers(kw, W, need):
    srv = _server(W, **kw)
    wires = [torch.zeros(srv.n, dtype=torch.float16) for _ in range(W)]
    with pytest.raises(ValueError, match=f"at least {need} sources, this round has {W}"):
        srv.update_range(wires, 1.0 / W, 0, srv.n)


def test_mean_hands_the_rule_the_same_list(monkeypatch):
    srv = _server(3)
    seen = []
    monkeypatch.setattr(type(srv.rule), "host", lambda self, s, srcs, *a: seen.append(srcs))
    wires = [torch.zeros(srv.n, dtype=torch.float16) for _ in range(3)]
    srv.update_range(wires, 1.0 / 3, 0, srv.n)
    assert seen[0] is wires and srv._robust is None and "robust_aggregate" not in srv.final_metrics()


def test_in_process_round_is_combined_not_summed():
    srv, ref = _server(3, aggregate="median"), _server(3)
    for s in (srv, ref):
        for w in range(3):
            s.register_worker(f"w{w}", w)
    g = torch.randn(srv.n, generator=torch.Generator().manual_seed(2)).half()
    for w, wire in enumerate([g, g, 1e4 * g]):  # the median of {g, g, 1e4 g} is g
        srv.push_gradients(w, wire.clone(), 0)
    for w in range(3):
        ref.push_gradients(w, g.clone(), 0)  # the mean of three g: g up to the fp32 sum's rounding
    assert torch.allclose(srv.params, ref.params, rtol=0, atol=1e-6)
    assert srv.final_metrics()["robust_aggregate"] == {"kind": "median", "rounds": 1}
