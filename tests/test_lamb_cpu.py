"""--optimizer lamb on the CPU path: configuration scope, the paths that decline it, the torch
implementation of the update in ParameterServer against an fp64 reference written here from the
formula, partial ranges, checkpoint / resume and the metrics keys. The reference (lamb_reference)
and its bounds (assert_lamb_close) are shared with the GPU kernel tests."""
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.ops import kernels as K
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

from .test_adamw_cpu import adamw_reference, wires
from .test_ps_cpu import tiny_cfg

U = 2.0 ** -24  # fp32 unit roundoff


def f32(x) -> float:
    return float(np.float32(x))


def fma32(a, b, c):
    """fp32 a * b + c with one rounding, element-wise on fp32 tensors (b may be a Python float
    holding an fp32 value). The product of two fp32 values is exact in fp64; the fp64 sum rounds
    once to 53 bits and once more to 24, which differs from the single rounding only when the fp64
    sum lands exactly on the midpoint of two fp32 values: those elements are redone in rationals."""
    a64 = a.double() * (b.double() if torch.is_tensor(b) else float(b))
    d = (a64 + c.double()).numpy()
    out = d.astype(np.float32)
    tie = (d.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)
    if tie.any():
        bb = b.double().numpy() if torch.is_tensor(b) else np.full(d.shape, float(b))
        an, cn = a.double().numpy(), c.double().numpy()
        for i in np.flatnonzero(tie):
            exact = Fraction(float(an[i])) * Fraction(float(bb[i])) + Fraction(float(cn[i]))
            lo, hi = sorted((np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))))
            cands = [lo, out[i], hi]
            best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.float32(x).view(np.int32)) & 1))
            out[i] = best
    return torch.from_numpy(out)


def lamb_reference(layout, p, m, v, s, scalars, gscale, wd):
    """One LAMB update in fp64, straight from the formulas, starting from the same fp32 p, m, v, s
    (the fp32 sum of the decoded worker gradients) and the same fp32 scalars (K.lamb_scalars:
    bc1 = 1 / (1 - beta1^t) rounded, beta1, 1 - beta1, beta2, 1 - beta2, rsqrt_bc2, eps) and fp32
    gscale and wd as the code under test:

        g  = gscale * s
        m' = beta1 m + (1 - beta1) g
        v' = beta2 v + (1 - beta2) g g
        r  = bc1 * m' / (sqrt(v') * rsqrt_bc2 + eps)
        u  = r + wd * w,  phi = |w| / |u| (1 if a norm is 0)     tensors with ndim > 1
        u  = r,           phi = 1                                 1-D tensors

    It takes no lr (p' = p - lr * phi * u is one fma of u and phi). Returns a dict: u, m, v (fp64),
    phi {name: ratio}, mag = |r| + wd |w| (0 * |w| for 1-D tensors), M and den as adamw_reference
    returns them, bc1, and k = the number of fp32 roundings lamb_tail.hpp adds after the quotient
    (2 for adapted tensors: the product with bc1 and the fma with wd * w; 1 for 1-D tensors).

    The bound on u (assert_lamb_close), with U = 2^-24: the quotient m' / den carries 4U (m',
    relative to M) + 2.5U (sqrt of v') + U (den) + U (divide), the product with bc1 U more —
    adamw_reference's derivation of its step, about 12U of bc1 M / den with the last fma it also
    counts; that term is used as derived, without adamw_reference's 3-4x margin. Each of the k
    roundings after the quotient adds U of |r| + wd |w|. So
        |u - u_ref| <= 12 U bc1 M / den + k U (|r| + wd |w|),
    relative to magnitudes, not to the result, so it holds whatever the signs of r and w."""
    bc1 = float(scalars[0])
    sc = [1.0] + [float(x) for x in scalars[1:7]] + [1.0]
    _, m2, v2, M, den = adamw_reference(p, m, v, s, sc, gscale)
    pd = p.double()
    r = bc1 * m2 / den
    u = r.clone()
    mag = r.abs()
    k = torch.ones_like(r)
    phi = {}
    for e in layout.entries.values():
        if e.region != "param" or not e.numel:
            continue
        sl = slice(e.offset, e.offset + e.numel)
        phi[e.name] = 1.0
        if len(e.shape) > 1:
            u[sl] = r[sl] + float(wd) * pd[sl]
            mag[sl] = r[sl].abs() + float(wd) * pd[sl].abs()
            k[sl] = 2.0
            wn, un = float(pd[sl].square().sum().sqrt()), float(u[sl].square().sum().sqrt())
            if wn > 0 and un > 0:
                phi[e.name] = wn / un
    return dict(u=u, m=m2, v=v2, phi=phi, mag=mag, M=M, den=den, bc1=bc1, k=k)


def assert_lamb_close(u_new, m_new, v_new, ref, what="", margin=1.0):
    """m', v' within adamw_reference's bounds, u within the bound of lamb_reference's docstring
    (times ``margin``); returns the worst error / bound of u."""
    for name, got, want, tol in (("m", m_new, ref["m"], 1e-6 * ref["M"]), ("v", v_new, ref["v"], 1e-6 * ref["v"])):
        err = (got.double().cpu() - want).abs()
        assert not bool((err > tol).any()), (what, name, float((err - tol).max()))
    tol = margin * (12 * U * ref["bc1"] * ref["M"] / ref["den"] + ref["k"] * U * ref["mag"])
    err = (u_new.double().cpu() - ref["u"]).abs()
    bad = err > tol
    assert not bool(bad.any()), (what, "u", int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()))
    return float((err / tol.clamp_min(1e-300)).max())


def test_fma32():
    a = torch.tensor([1.0 + 2.0 ** -23, 3.0, 1.0 + 2.0 ** -12], dtype=torch.float32)
    b = torch.tensor([1.0 + 2.0 ** -23, 0.5, 1.0 + 2.0 ** -12], dtype=torch.float32)
    c = torch.tensor([-1.0, 2.0 ** -30, 2.0 ** -25], dtype=torch.float32)
    want = [float(np.float32(float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))))
            for x, y, z in zip(a, b, c)]
    assert fma32(a, b, c).tolist() == want
    # double rounding: a * b = 2^-24 - 2^-54, c = 1 + 2^-23 (odd mantissa). The exact sum is just below
    # the midpoint of c and its successor (rounds to c); the fp64 sum is that midpoint, and rounds
    # to even, away from c
    a = torch.tensor([2.0 ** -12 * (1 + 2.0 ** -15)], dtype=torch.float32)
    b = torch.tensor([2.0 ** -12 * (1 - 2.0 ** -15)], dtype=torch.float32)
    c = torch.tensor([1.0 + 2.0 ** -23], dtype=torch.float32)
    assert float(np.float32(float(a) * float(b) + float(c))) == 1.0 + 2.0 ** -22
    assert float(fma32(a, b, c)[0]) == 1.0 + 2.0 ** -23
    assert float(fma32(a, float(b), c)[0]) == 1.0 + 2.0 ** -23


def test_reference_is_torch_adam():
    """On 1-D tensors with wd = 0 LAMB is Adam: five steps against torch.optim.Adam in float64,
    the scalars computed in double from exact betas."""
    from psx.models.layout import Entry

    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    lay = ParamLayout()
    lay.entries["a"] = Entry("a", (600,), "float32", "param", 0, 600)
    lay.entries["b"] = Entry("b", (400,), "float32", "param", 600, 400)
    lay.param_numel = 1000
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(1000, dtype=torch.float64, generator=gen) * 0.05
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, 6):
        g = torch.randn(1000, dtype=torch.float64, generator=gen) * 1e-2
        q.grad = g.clone()
        opt.step()
        exact = (1 / (1 - b1 ** t), b1, 1 - b1, b2, 1 - b2, 1 / np.sqrt(1 - b2 ** t), eps, 1.0)
        ref = lamb_reference(lay, p, m, v, g, exact, 1.0, 0.0)
        assert set(ref["phi"].values()) == {1.0}
        p, m, v = p - lr * ref["u"], ref["m"], ref["v"]
    assert float((p - q.detach()).abs().max()) <= 1e-12


def test_scalars():
    for t in (1, 2, 1000):
        a = K.lamb_scalars(t)
        assert a == K.lamb_scalars_host(t) == K.adamw_scalars(1.0, t, wd=0.0)
        assert a[0] == f32(1 / (1 - 0.9 ** t)) and a[7] == 1.0


# ---------------------------------------------------------------------------- configuration
def test_config_scope():
    cfg = PSConfig(optimizer="lamb").validate()
    assert (cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps) == (0.9, 0.999, 1e-8)
    d = PSConfig().validate()
    assert d.optimizer == "sgd" and d.warmup_steps == 0
    for bad in (dict(adam_beta1=1.0), dict(adam_beta1=-0.1), dict(adam_beta2=1.0), dict(adam_beta2=-1e-3),
                dict(adam_eps=0.0), dict(adam_eps=-1e-8), dict(momentum=0.9), dict(topology="sharded", mode="sync"),
                dict(overlap=True), dict(mode="async", dc_lambda=0.04), dict(clip_norm=1.0),
                dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="--optimizer lamb"):
            PSConfig(optimizer="lamb", **bad).validate()
    PSConfig(optimizer="lamb", adam_beta1=0.0, adam_beta2=0.0).validate()
    assert PSConfig(mode="sync", optimizer="lamb").validate().resolve_overlap(8) is False
    assert PSConfig(mode="sync").validate().resolve_overlap(8) is True


def test_cli_flags():
    from psx.utils.config import parse

    cfg = parse(["--optimizer", "lamb", "--adam-beta1", "0.8", "--adam-beta2", "0.99", "--adam-eps", "1e-6",
                 "--weight-decay", "1e-2", "--lr", "2e-3", "--warmup-steps", "7"])
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay, cfg.lr, cfg.warmup_steps) \
        == ("lamb", 0.8, 0.99, 1e-6, 1e-2, 2e-3, 7)
    d = parse(["--optimizer", "lamb"])
    assert (d.adam_beta1, d.adam_beta2, d.adam_eps, d.warmup_steps) == (0.9, 0.999, 1e-8, 0)


def test_native_paths_decline_lamb(monkeypatch):
    """The native C++ loops, the captured graph round and the elastic shrink serve the SGD server
    only; under lamb the same stubs select the Python server (or the constructors refuse)."""
    from psx.parallel import elastic
    from psx.parallel.graph_round import graph_round_enabled
    from psx.parallel.native_loop import NativeServerLoop, native_loop_enabled
    from psx.parallel.native_sync import NativeSyncServer, native_sync_enabled
    from psx.parallel.runner import run_local_threads
    from psx.parallel.worker import SyncCollectiveChannel

    for k in ("PSX_NATIVE_LOOP", "PSX_NATIVE_SYNC", "PSX_SYNC_AGG"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PSX_GRAPH_ROUND", "1")
    t = types.SimpleNamespace(native=True, world_size=3, rank=0)
    srv = types.SimpleNamespace(wire=None)
    for opt, want in (("sgd", True), ("lamb", False)):
        a = PSConfig(mode="async", optimizer=opt).validate()
        assert native_loop_enabled(a, t) is want
        s = PSConfig(mode="sync", topology="dedicated", optimizer=opt).validate()
        chan = SyncCollectiveChannel(t, srv, members=[0, 1], codec=None, root_worker=False)
        assert native_sync_enabled(s, t, chan, srv, 0) is want
        assert elastic.enabled(s, t, 3) is want
        c = PSConfig(mode="sync", topology="colocated", optimizer=opt).validate()
        assert graph_round_enabled(c, t) is want
    lamb = PSConfig(mode="async", optimizer="lamb").validate()
    stub = types.SimpleNamespace(cfg=lamb, layout=None, device="cpu")
    with pytest.raises(ValueError, match="--optimizer lamb"):
        NativeServerLoop(stub, None, None, {}, 1)
    with pytest.raises(ValueError, match="--optimizer lamb"):
        NativeSyncServer(stub, t, None)
    with pytest.raises(ValueError, match="--optimizer lamb"):
        run_local_threads(lamb, 1)


# ---------------------------------------------------------------------------- server numerics
HP = dict(lr=2e-3, weight_decay=1e-2)


def tiny_server(optimizer="lamb", device="cpu", **kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(**{**dict(mode="async", workers=1, optimizer=optimizer), **HP, **kw})
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=cfg.workers,
                        log=lambda *a: None)
    for w in range(cfg.workers):
        s.register_worker("w", w)
    return s, lay, cfg


def server_scalars(cfg, t):
    return K.lamb_scalars(t, beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_eps)


def server_step_reference(s, lay, cfg, dense, weight):
    """The fp64 reference of the server's next update from its current state: (ref, p_ref)."""
    ref = lamb_reference(lay, s.params.cpu(), s.adam_m.cpu(), s.adam_v.cpu(), dense.cpu(),
                         server_scalars(cfg, s.adam_t + 1), f32(weight), f32(cfg.weight_decay))
    step = torch.ones(lay.param_numel, dtype=torch.float64)
    for e in lay.entries.values():
        if e.region == "param" and e.numel:
            step[e.offset:e.offset + e.numel] = ref["phi"][e.name]
    return ref, s.params.cpu().double() - f32(s.lr) * step * ref["u"]


def assert_server_step(s, lay, ref, p_ref, p_old, lr, what=""):
    """Moments within adamw_reference's bounds; the parameter step within the u bound scaled by
    lr * phi, plus 2e-5 of the step for the ratio (the norms' reduction order) and the roundings
    of lr * phi and of the final subtraction."""
    for name, got, want, tol in (("m", s.adam_m, ref["m"], 1e-6 * ref["M"]),
                                 ("v", s.adam_v, ref["v"], 1e-6 * ref["v"])):
        assert not bool(((got.double().cpu() - want).abs() > tol).any()), (what, name)
    d_ref = p_ref - p_old.double()
    utol = 12 * U * ref["bc1"] * ref["M"] / ref["den"] + ref["k"] * U * ref["mag"]
    scale = (d_ref.abs() / ref["u"].abs().clamp_min(1e-300))  # lr * phi per element
    tol = scale * utol + 2e-5 * d_ref.abs() + 2.0 ** -23 * p_old.double().abs()
    err = (s.params.double().cpu() - p_ref).abs()
    assert not bool((err > tol).any()), (what, "p", float((err / tol.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("kind", ["fp16", "q8", "topk"])
def test_server_apply_matches_reference(kind):
    """ParameterServer.apply on a CPU arena, four consecutive pushes, against the fp64 reference
    applied to the decoded gradient; 1-D tensors take ratio 1 and no decay."""
    s, lay, cfg = tiny_server(codec=kind, topk_ratio=0.25)
    for step, (wire, dense) in enumerate(wires(kind, lay.param_numel, 4, cfg)):
        assert s.adam_t == step
        p_old = s.params.clone()
        ref, p_ref = server_step_reference(s, lay, cfg, dense, 0.5)
        s.apply(wire, 0.5)
        assert_server_step(s, lay, ref, p_ref, p_old, cfg.lr, (kind, step))
        assert not torch.equal(s.params, p_old)
        adapted = [ref["phi"][e.name] for e in lay.entries.values() if e.region == "param" and len(e.shape) > 1]
        assert s._lamb_ratios == pytest.approx(adapted, rel=1e-5)
        assert all(ref["phi"][e.name] == 1.0 for e in lay.entries.values() if e.region == "param" and len(e.shape) == 1)
    assert s.core.global_step == 4 and s.adam_t == 4
    fm = s.final_metrics()
    assert fm["optimizer"] == "lamb"
    assert fm["lamb"] == {"beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "steps": 4}
    r = torch.tensor(adapted)
    assert fm["lamb_trust_ratio"] == pytest.approx({"min": float(r.min()), "median": float(r.median()),
                                                    "max": float(r.max())}, rel=1e-5)


def test_one_d_tensors_take_no_decay():
    """A 1-D tensor's update is independent of --weight-decay; an adapted tensor's is not."""
    a, lay, cfg = tiny_server(codec="none")
    b, _, _ = tiny_server(codec="none", weight_decay=0.0)
    g = torch.randn(lay.param_numel, generator=torch.Generator().manual_seed(4)) * 1e-2
    a.apply(g, 1.0)
    b.apply(g, 1.0)
    seen = set()
    for e in lay.entries.values():
        if e.region != "param" or not e.numel:
            continue
        same = torch.equal(a.params[e.offset:e.offset + e.numel], b.params[e.offset:e.offset + e.numel])
        assert same == (len(e.shape) == 1), e.name
        seen.add(len(e.shape) == 1)
    assert seen == {True, False}


def test_sync_round_of_three_fp16_wires():
    """W = 3 fp16 wires through apply_sources: the fp32 source-order sum, weight 1 / 3."""
    s, lay, cfg = tiny_server(mode="sync", workers=3)
    gen = torch.Generator().manual_seed(6)
    for rnd in range(3):
        srcs = [(torch.randn(lay.param_numel, generator=gen) * 1e-2).half() for _ in range(3)]
        dense = torch.zeros(lay.param_numel)
        for x in srcs:
            dense = dense + x.float()
        p_old = s.params.clone()
        ref, p_ref = server_step_reference(s, lay, cfg, dense, 1.0 / 3)
        assert s.apply_sources(srcs, [0, 1, 2], [rnd + 1] * 3)
        assert_server_step(s, lay, ref, p_ref, p_old, cfg.lr, rnd)
    assert s.adam_t == 3


def test_partial_range_raises():
    s, lay, _ = tiny_server(codec="fp16")
    n = lay.param_numel
    g = torch.zeros(n).half()
    with pytest.raises(ValueError, match="--optimizer lamb"):
        s.apply_range(g[: n // 2], 1.0, 0, n // 2)
    with pytest.raises(ValueError, match="--optimizer lamb"):
        s.apply_range_sources([g], 1.0, 8, n)
    assert s.adam_t == 0 and not bool(s.adam_m.any())


def test_wire_goes_stale_on_a_cpu_arena():
    s, lay, _ = tiny_server(codec="fp16")
    s.enable_weight_wire()
    assert not s._wire_stale
    s.apply(torch.zeros(lay.param_numel).half(), 1.0)
    assert s._wire_stale


def test_checkpoint_resume(tmp_path):
    kw = dict(codec="none", ckpt_dir=str(tmp_path))
    a, lay, _ = tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2, g3 = (torch.randn(lay.param_numel, generator=gen) * 1e-2 for _ in range(3))
    a.apply(g1, 1.0)
    path = a.checkpoint()
    a.apply(g2, 1.0)
    a.apply(g3, 1.0)
    b, _, _ = tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 1 and b.adam_t == 1
    b.apply(g2, 1.0)
    b.apply(g3, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert a.adam_t == b.adam_t == 3


def test_run_local_sync_lamb():
    from psx.parallel.runner import run_local

    cfg = tiny_cfg(mode="sync", workers=2, optimizer="lamb", eval_every=0, **HP)
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    assert srv["optimizer"] == "lamb" and srv["global_steps_completed"] > 0
    assert srv["lamb"]["steps"] == srv["global_steps_completed"]
    assert set(srv["lamb_trust_ratio"]) == {"min", "median", "max"}
    assert np.isfinite(srv["final_param_checksum"])
