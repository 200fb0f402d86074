"""ParameterServer with --optimizer lamb on the device, resnet_tiny's layout: the fp64 reference
chain over four rounds, q8 and top-k payloads through the dense entry, the weight image, and
checkpoint / resume."""
import pytest
import torch

from psx.ops import kernels as K

from .test_adamw_cpu import wires
from .test_lamb_cpu import assert_lamb_close, fma32, server_step_reference, tiny_server

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _spy(monkeypatch):
    calls = []
    for name in ("lamb_apply", "lamb_apply_multi"):
        fn = getattr(K, name)

        def wrap(*a, _fn=fn, _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)

        monkeypatch.setattr(K, name, wrap)
    return calls


@pytest.mark.parametrize("kind,entry", [("fp16", "lamb_apply_multi"), ("q8", "lamb_apply"), ("topk", "lamb_apply")])
def test_device_server_matches_reference_chain(kind, entry, monkeypatch):
    """Four consecutive pushes: every round's moments, u (left in the aggregation buffer) and
    ratios against the fp64 reference started from the device's state before the round, and p' the
    one fma of the device's u and ratio. The fp16 wire takes the multi-source entry, q8 and top-k
    payloads are decoded into the aggregation buffer and take the dense one."""
    calls = _spy(monkeypatch)
    s, lay, cfg = tiny_server(device=DEV, codec=kind, topk_ratio=0.25)
    tab = s._lars_tab
    for step, (wire, dense) in enumerate(wires(kind, lay.param_numel, 4, cfg, device=DEV)):
        p_old = s.params.cpu()
        ref, _ = server_step_reference(s, lay, cfg, dense, 0.5)
        s.apply(wire, 0.5)
        torch.cuda.synchronize()
        assert_lamb_close(s.agg, s.adam_m, s.adam_v, ref, (kind, step))
        lam = tab.ratios.cpu()
        want = torch.tensor([ref["phi"][nm] for nm in tab.names], dtype=torch.float64)
        assert bool(((lam.double() - want).abs() <= 1e-5 * want.abs()).all()), (kind, step)
        assert all(float(lam[i]) == 1.0 for i, a in enumerate(tab.adapt) if not a)
        step32 = torch.empty(lay.param_numel)
        lr = torch.tensor(cfg.lr, dtype=torch.float32)
        for nm, phi in zip(tab.names, lam):
            e = lay.entries[nm]
            step32[e.offset:e.offset + e.numel] = lr * phi
        assert torch.equal(s.params.cpu().view(torch.int32), fma32(s.agg.cpu(), -step32, p_old).view(torch.int32))
    assert calls == [entry] * 4 and s.adam_t == 4 and s.core.global_step == 4
    fm = s.final_metrics()
    assert fm["optimizer"] == "lamb" and fm["lamb"]["steps"] == 4
    r = lam[torch.tensor(tab.adapt)]
    assert fm["lamb_trust_ratio"] == {"min": float(r.min()), "median": float(r.median()), "max": float(r.max())}


def test_accumulated_round_takes_the_dense_entry(monkeypatch):
    """A loopback sync round of two workers is summed into the aggregation buffer and applied
    through the dense entry: the bits of the same two wires through the multi-source entry."""
    calls = _spy(monkeypatch)
    a, lay, cfg = tiny_server(device=DEV, mode="sync", workers=2, codec="fp16")
    b, _, _ = tiny_server(device=DEV, mode="sync", workers=2, codec="fp16")
    gen = torch.Generator().manual_seed(12)
    for rnd in range(2):
        g0, g1 = ((torch.randn(lay.param_numel, generator=gen) * 1e-2).half().to(DEV) for _ in range(2))
        a.push_gradients(0, g0, rnd + 1)
        a.push_gradients(1, g1, rnd + 1)
        assert b.apply_sources([g0, g1], [0, 1], [rnd + 1] * 2)
    assert a.core.global_step == b.core.global_step == 2, (a.core.global_step, b.core.global_step)
    assert calls == ["lamb_apply", "lamb_apply_multi"] * 2
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)


def test_weight_image():
    """With the weight-image fetch path on, the LAMB apply writes the bf16 image of the updated
    parameters in the same pass (no stale wire)."""
    s, lay, _ = tiny_server(device=DEV, codec="fp16", dtype="bf16")
    s.enable_weight_wire()
    before = s.params.clone()
    s.apply((torch.randn(lay.param_numel, generator=torch.Generator().manual_seed(3)) * 1e-2).half().to(DEV), 1.0)
    assert not s._wire_stale and not torch.equal(before, s.params)
    assert torch.equal(s.wire.img[: lay.param_numel], s.params.bfloat16())


def test_checkpoint_resume_is_bit_identical(tmp_path):
    kw = dict(device=DEV, codec="fp16", ckpt_dir=str(tmp_path))
    a, lay, _ = tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    gs = [(torch.randn(lay.param_numel, generator=gen) * 1e-2).half().to(DEV) for _ in range(4)]
    for g in gs[:2]:
        a.apply(g, 1.0)
    path = a.checkpoint()
    for g in gs[2:]:
        a.apply(g, 1.0)
    b, _, _ = tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 2 and b.adam_t == 2
    for g in gs[2:]:
        b.apply(g, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert a.adam_t == b.adam_t == 4
    assert a.final_metrics()["final_param_sha256"] == b.final_metrics()["final_param_sha256"]
