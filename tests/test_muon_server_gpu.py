"""ParameterServer with --optimizer muon --momentum 0.95 on the device, resnet_tiny's layout: four
rounds of two workers against the CPU-arena server (the rule's torch form) fed the same rounds;
fp16 wires take the multi-source entry, q8 payloads the dense one."""
import pytest
import torch

from psx.ops import kernels as K

from .test_adamw_cpu import wires
from .test_lamb_cpu import tiny_server
from .test_muon_cpu import chain_yardstick, matrices

pytestmark = pytest.mark.gpu

ROUNDS = 4


@pytest.mark.parametrize("kind,entry", [("fp16", "muon_apply_multi"), ("q8", "muon_apply")])
def test_device_server_matches_cpu_server(kind, entry, monkeypatch):
    """Per element and round, within lr x sqrt(max(1, rows / cols)) x 4 x the chain yardstick (the
    torch fp32 chain's own error on that round's u, momentum included; the direction of a Muon
    step does not depend on w, so the two servers' steps do not drift apart). Beyond the issue's
    bound, since both sides store w in fp32: 2^-22 |w| and 2^-21 |step| per round, test_muon_cpu's
    update_bound allowance once for each of the two fp32 implementations compared."""
    calls = []
    fn = getattr(K, entry)
    monkeypatch.setattr(K, entry, lambda *a, **kw: (calls.append(entry), fn(*a, **kw))[1])
    kw = dict(optimizer="muon", momentum=0.95, mode="sync", workers=2, codec=kind, lr=0.02)
    d, lay, cfg = tiny_server(device="cuda", **kw)
    c, _, _ = tiny_server(**kw)
    n = lay.param_numel
    pushes = [wires(kind, n, ROUNDS, cfg, device="cuda", seed=sd) for sd in (11, 12)]
    moved, yards = torch.zeros(n, dtype=torch.float64), 0.0
    for rnd in range(ROUNDS):
        srcs, before = [pushes[w][rnd][0] for w in range(2)], c.params.double()
        assert d.apply_sources(srcs, [0, 1], [rnd + 1] * 2)
        assert c.apply_sources([s.cpu() for s in srcs], [0, 1], [rnd + 1] * 2)
        moved += (c.params.double() - before).abs()
        g = 0.5 * (pushes[0][rnd][1] + pushes[1][rnd][1]).cpu()
        yards += chain_yardstick(matrices(lay, g + 0.95 * c.momentum_buf))
    assert calls == [entry] * ROUNDS
    scale = torch.zeros(n, dtype=torch.float64)
    for e in lay.entries.values():
        if e.region == "param" and len(e.shape) > 1:
            scale[e.offset:e.offset + e.numel] = max(1.0, e.shape[0] ** 2 / e.numel) ** 0.5
    tol = cfg.lr * 4 * yards * scale + ROUNDS * 2.0 ** -22 * c.params.double().abs() + 2.0 ** -21 * moved
    err = (d.params.cpu().double() - c.params.double()).abs()
    assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())
    assert torch.allclose(d.momentum_buf.cpu(), c.momentum_buf, rtol=1e-5, atol=1e-8)
    fm = d.final_metrics()
    assert fm["optimizer"] == "muon" and set(fm["muon_update_norm"]) == {"min", "median", "max"}
