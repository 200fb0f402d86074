"""--optimizer adamw on the CPU path: configuration scope, the paths that decline it, the torch
implementation of the update in ParameterServer against an fp64 reference written here from the
formula, ranges, checkpoint / resume and end-to-end runs. The reference (adamw_reference) and its
bounds (assert_adamw_close) are shared with the GPU kernel tests."""
import types

import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.ops import kernels as K
from psx.parallel import q8 as Q
from psx.parallel import topk as T
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

from .test_ps_cpu import TINY, _spawn, tiny_cfg


def f32(x) -> float:
    return float(np.float32(x))


def adamw_reference(p, m, v, s, scalars, gscale):
    """One AdamW update in fp64, straight from the formula, starting from the same fp32 p, m, v,
    s (the fp32 sum of the decoded worker gradients) and the same eight scalars (step_size, beta1,
    1 - beta1, beta2, 1 - beta2, rsqrt_bc2, eps, decay) as the code under test:

        g  = s * gscale
        m' = beta1 * m + (1 - beta1) * g
        v' = beta2 * v + (1 - beta2) * g * g
        p' = p * decay - step_size * m' / (sqrt(v') * rsqrt_bc2 + eps)

    Returns (p', m', v', M, den) in fp64 with M = beta1 |m| + (1 - beta1) |g| and den = sqrt(v') *
    rsqrt_bc2 + eps, the magnitudes the bounds of assert_adamw_close are relative to.

    The bounds, with u = 2^-24 (fp32 unit roundoff). The fp32 chain is product (g), product, fma
    (m'), square, product, fma (v'), sqrt, fma (den), divide, product, fma (p'):
      * m': at most 4u relative to M (g, (1-beta1) g and the fma round once each, every error
        bounded by its term's magnitude, which M sums)             -> bound 1e-6 M    (~17u)
      * v': all terms are >= 0, so about 5u relative to v' itself  -> bound 1e-6 v'
      * the step m'/den: 4u (m') + 2.5u (sqrt of v') + u (den) + u (divide) + u (product with
        step_size) + the fma, about 12u of step_size M / den       -> bound 2e-6 step_size M / den (~34u)
      * p: u |p| from p * decay and u |p'| from the final rounding -> bound 2^-22 |p|    (4u)
    The bounds keep a 3-4x margin over the derivation and are relative to magnitude sums, so they
    hold whatever the signs of p, m and g. With exact (double) hyper-parameters this form equals
    torch.optim.AdamW in float64 to ~1e-17 (test_reference_is_torch_adamw)."""
    step_size, b1, omb1, b2, omb2, rbc2, eps, decay = (float(x) for x in scalars)
    p, m, v, s = (x.double() for x in (p, m, v, s))
    g = s * float(gscale)
    M = b1 * m.abs() + omb1 * g.abs()
    m2 = b1 * m + omb1 * g
    v2 = b2 * v + omb2 * g * g
    den = v2.sqrt() * rbc2 + eps
    return p * decay - step_size * m2 / den, m2, v2, M, den


def assert_adamw_close(p_new, m_new, v_new, p_old, ref, scalars, what=""):
    """The bounds of adamw_reference's docstring; returns the worst error / bound of (m, v, p)."""
    p_ref, m_ref, v_ref, M, den = ref
    step = float(scalars[0])
    worst = []
    for name, got, want, tol in (
            ("m", m_new, m_ref, 1e-6 * M),
            ("v", v_new, v_ref, 1e-6 * v_ref),
            ("p", p_new, p_ref, 2.0 ** -22 * p_old.double().abs() + 2e-6 * step * M / den)):
        err = (got.double().cpu() - want).abs()
        bad = err > tol
        assert not bool(bad.any()), (what, name, int(bad.sum()), float((err - tol).max()))
        worst.append(float((err / tol.clamp_min(1e-300)).max()))
    return worst


def test_reference_is_torch_adamw():
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(1000, dtype=torch.float64, generator=gen) * 0.05
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, 6):
        g = torch.randn(1000, dtype=torch.float64, generator=gen) * 1e-2
        q.grad = g.clone()
        opt.step()
        exact = (lr / (1 - b1 ** t), b1, 1 - b1, b2, 1 - b2, 1 / np.sqrt(1 - b2 ** t), eps, 1 - lr * wd)
        p, m, v, _, _ = adamw_reference(p, m, v, g, exact, 1.0)
    assert float((p - q.detach()).abs().max()) <= 1e-12


def test_scalars():
    """The library's scalars (the values the kernel receives) and the Python form agree bit for bit."""
    for t in (1, 2, 7, 1000, 100000):
        for kw in (dict(), dict(beta1=0.0, beta2=0.5, eps=1e-6, wd=1e-2)):
            a = K.adamw_scalars(1e-3, t, **kw)
            assert a == K.adamw_scalars_host(1e-3, t, **kw) and len(a) == 8
            assert all(x == f32(x) for x in a)
    b1, b2 = 0.9, 0.999
    a = K.adamw_scalars(1e-3, 3, wd=1e-2)
    assert a == [f32(1e-3 / (1 - b1 ** 3)), f32(b1), f32(1 - b1), f32(b2), f32(1 - b2),
                 f32(1 / np.sqrt(1 - b2 ** 3)), f32(1e-8), f32(1 - 1e-3 * 1e-2)]


# ---------------------------------------------------------------------------- configuration
def test_config_scope():
    cfg = PSConfig(optimizer="adamw").validate()
    assert (cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps) == (0.9, 0.999, 1e-8)
    with pytest.raises(ValueError):
        PSConfig(optimizer="adam").validate()
    for bad in (dict(adam_beta1=1.0), dict(adam_beta1=-0.1), dict(adam_beta2=1.0), dict(adam_beta2=-1e-3),
                dict(adam_eps=0.0), dict(adam_eps=-1e-8)):
        with pytest.raises(ValueError, match="--optimizer adamw"):
            PSConfig(optimizer="adamw", **bad).validate()
    PSConfig(optimizer="adamw", adam_beta1=0.0, adam_beta2=0.0).validate()
    with pytest.raises(ValueError, match="--optimizer adamw"):
        PSConfig(optimizer="adamw", momentum=0.9).validate()
    with pytest.raises(ValueError, match="--optimizer adamw"):
        PSConfig(optimizer="adamw", mode="async", dc_lambda=0.04).validate()
    with pytest.raises(ValueError, match="--optimizer adamw"):
        PSConfig(optimizer="adamw", clip_norm=1.0).validate()
    with pytest.raises(ValueError, match="--optimizer adamw"):
        PSConfig(optimizer="adamw", skip_nonfinite=True).validate()
    PSConfig(optimizer="adamw", mode="sync", topology="sharded").validate()
    assert PSConfig(optimizer="adamw", mode="sync", overlap=True).validate().resolve_overlap(8) is True
    assert PSConfig(optimizer="adamw", mode="sync").validate().resolve_overlap(8) is True


def test_cli_flags():
    from psx.utils.config import parse

    cfg = parse(["--optimizer", "adamw", "--adam-beta1", "0.8", "--adam-beta2", "0.99", "--adam-eps", "1e-6",
                 "--weight-decay", "1e-2", "--lr", "1e-3"])
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay, cfg.lr) == \
        ("adamw", 0.8, 0.99, 1e-6, 1e-2, 1e-3)
    d = parse(["--optimizer", "adamw"])
    assert (d.adam_beta1, d.adam_beta2, d.adam_eps) == (0.9, 0.999, 1e-8)


def test_native_paths_decline_adamw(monkeypatch):
    """The native C++ loops, the captured graph round and the elastic shrink serve the SGD server
    only; under adamw the same stubs select the Python server (or the constructors refuse)."""
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
    for opt, want in (("sgd", True), ("adamw", False)):
        a = PSConfig(mode="async", optimizer=opt).validate()
        assert native_loop_enabled(a, t) is want
        s = PSConfig(mode="sync", topology="dedicated", optimizer=opt).validate()
        chan = SyncCollectiveChannel(t, srv, members=[0, 1], codec=None, root_worker=False)
        assert native_sync_enabled(s, t, chan, srv, 0) is want
        assert elastic.enabled(s, t, 3) is want
        c = PSConfig(mode="sync", topology="colocated", optimizer=opt).validate()
        assert graph_round_enabled(c, t) is want
    adamw = PSConfig(mode="async", optimizer="adamw").validate()
    stub = types.SimpleNamespace(cfg=adamw, layout=None, device="cpu")
    with pytest.raises(ValueError, match="--optimizer adamw"):
        NativeServerLoop(stub, None, None, {}, 1)
    with pytest.raises(ValueError, match="--optimizer adamw"):
        NativeSyncServer(stub, t, None)
    with pytest.raises(ValueError, match="--optimizer adamw"):
        run_local_threads(adamw, 1)


# ---------------------------------------------------------------------------- server numerics
HP = dict(lr=1e-3, weight_decay=1e-2)


def _tiny_server(optimizer="adamw", device="cpu", **kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(**{**dict(mode="async", workers=1, optimizer=optimizer), **HP, **kw})
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=1, log=lambda *a: None)
    s.register_worker("w", 0)
    return s, lay, cfg


def server_scalars(cfg, t):
    return K.adamw_scalars(cfg.lr, t, beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_eps,
                           wd=cfg.weight_decay)


def wires(kind: str, n: int, steps: int, cfg, device="cpu", seed=11):
    """``steps`` pushes of one wire kind with the dense fp32 gradient each decodes to (random
    signs; the encoders start each push without residual)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    enc = Q.Q8Codec(n, device) if kind == "q8" else T.TopKCodec(n, cfg.topk_ratio, device) if kind == "topk" else None
    for _ in range(steps):
        g = (torch.randn(n, generator=gen) * 1e-2).to(device)
        if enc is not None:
            enc.resid.zero_()
        if kind == "fp16":
            wire = g.half()
            dense = wire.float()
        elif kind == "q8":
            wire = enc.encode(g).clone()
            dense = Q.decode(wire, n).clone()
        else:
            wire = enc.encode(g).clone()
            dense = T.decode_add(wire, torch.zeros(n, device=device), 1.0, T.topk_k(n, cfg.topk_ratio)).clone()
        out.append((wire, dense))
    return out


@pytest.mark.parametrize("kind", ["fp16", "q8", "topk"])
def test_server_apply_matches_reference(kind):
    """ParameterServer.apply on a CPU arena, three consecutive pushes (t = 1, 2, 3), against the
    fp64 reference applied to the decoded gradient."""
    s, lay, cfg = _tiny_server(codec=kind, topk_ratio=0.25)
    n = lay.param_numel
    for step, (wire, dense) in enumerate(wires(kind, n, 3, cfg)):
        assert s.adam_t == step
        sc = server_scalars(cfg, step + 1)
        p_old = s.params.clone()
        ref = adamw_reference(p_old, s.adam_m, s.adam_v, dense, sc, 0.5)
        s.apply(wire, 0.5)
        assert_adamw_close(s.params, s.adam_m, s.adam_v, p_old, ref, sc, (kind, step))
        assert not torch.equal(s.params, p_old)
    assert s.core.global_step == 3 and s.adam_t == 3
    fm = s.final_metrics()
    assert fm["optimizer"] == "adamw"
    assert fm["adamw"] == {"beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "steps": 3}


def test_topk_never_takes_the_stateless_scatter():
    """No momentum and no weight decay: the SGD server scatters a top-k payload straight into the
    parameters; AdamW must still go through its moments."""
    s, lay, cfg = _tiny_server(codec="topk", topk_ratio=0.25, weight_decay=0.0)
    (wire, dense), = wires("topk", lay.param_numel, 1, cfg)
    sc = server_scalars(cfg, 1)
    p_old = s.params.clone()
    ref = adamw_reference(p_old, s.adam_m, s.adam_v, dense, sc, 1.0)
    s.apply(wire, 1.0)
    assert_adamw_close(s.params, s.adam_m, s.adam_v, p_old, ref, sc)
    assert float(s.adam_v.abs().sum()) > 0


def test_ranges_equal_the_whole_round():
    """One round applied as three ranges [0,a), [a,b), [b,n) with odd a and b is bit-equal to the
    same round applied whole, and advances adam_t once."""
    a_srv, lay, cfg = _tiny_server(codec="fp16")
    b_srv, _, _ = _tiny_server(codec="fp16")
    n = lay.param_numel
    a, b = n // 3 | 1, (2 * n // 3) | 1
    assert a % 2 == 1 and b % 2 == 1 and 0 < a < b < n
    gen = torch.Generator().manual_seed(5)
    for rnd in range(2):
        srcs = [(torch.randn(n, generator=gen) * 1e-2).half() for _ in range(2)]
        a_srv.apply_range_sources(srcs, 0.5, 0, n)
        a_srv.finish_round_apply()
        for lo, hi in ((0, a), (a, b), (b, n)):
            b_srv.apply_range_sources(srcs, 0.5, lo, hi)
            assert b_srv.adam_t == rnd  # every range of the round shares t
        b_srv.finish_round_apply()
        assert a_srv.adam_t == b_srv.adam_t == rnd + 1
        assert torch.equal(a_srv.arena, b_srv.arena)
        assert torch.equal(a_srv.adam_m, b_srv.adam_m) and torch.equal(a_srv.adam_v, b_srv.adam_v)


def test_wire_goes_stale_on_a_cpu_arena():
    s, lay, cfg = _tiny_server(codec="fp16")
    s.enable_weight_wire()
    assert not s._wire_stale
    s.apply(torch.zeros(lay.param_numel).half(), 1.0)
    assert s._wire_stale


# ---------------------------------------------------------------------------- checkpoint / resume
def test_checkpoint_resume(tmp_path):
    kw = dict(codec="none", ckpt_dir=str(tmp_path))
    a, lay, _ = _tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2 = (torch.randn(lay.param_numel, generator=gen) * 1e-2 for _ in range(2))
    a.apply(g1, 1.0)
    path = a.checkpoint()
    a.apply(g2, 1.0)
    b, _, _ = _tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 1 and b.adam_t == 1
    b.apply(g2, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert a.adam_t == b.adam_t == 2


def test_sgd_checkpoint_loads_with_zero_state(tmp_path):
    kw = dict(codec="none", ckpt_dir=str(tmp_path))
    sgd, lay, _ = _tiny_server(optimizer="sgd", **kw)
    sgd.apply(torch.full((lay.param_numel,), 1e-2), 1.0)
    path = sgd.checkpoint()
    b, _, _ = _tiny_server(**kw)
    b.apply(torch.full((lay.param_numel,), 1e-2), 1.0)  # state to be discarded by the resume
    b.resume(path)
    assert torch.equal(b.arena, sgd.arena) and b.core.global_step == 1
    assert b.adam_t == 0 and not bool(b.adam_m.any()) and not bool(b.adam_v.any())


# ---------------------------------------------------------------------------- runs
def test_run_local_sync_adamw():
    from psx.parallel.runner import run_local

    cfg = tiny_cfg(mode="sync", workers=2, optimizer="adamw", eval_every=0, **HP)
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    assert srv["optimizer"] == "adamw" and srv["global_steps_completed"] > 0
    assert srv["adamw"]["steps"] == srv["global_steps_completed"]
    assert np.isfinite(srv["final_param_checksum"])


def test_dist_sync_gloo_matches_run_local():
    """Two gloo ranks (colocated, W = 2, the default bucketed round) against the loopback run of
    the same job: the assertion of test_ps_cpu.test_dist_sync_overlap_matches_serial."""
    from psx.parallel.runner import run_local

    args = ["--mode", "sync", "--optimizer", "adamw", "--weight-decay", "1e-2", "--eval-every", "0"]
    tiny = [x for x in TINY]
    tiny[tiny.index("--lr") + 1] = "1e-3"
    i = tiny.index("--eval-every")
    del tiny[i:i + 2]
    recs, _ = _spawn(2, args + tiny)
    srv = [r for r in recs if r["type"] == "SERVER_FINAL_METRICS"][0]
    # one thread, as the spawned ranks run (OMP_NUM_THREADS=1): Adam's first steps are close to
    # lr * sign(g), so the last-bit differences of another thread count's reduction order in the
    # workers' gradients do not stay last-bit differences of the parameters
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        loc = run_local(tiny_cfg(mode="sync", workers=2, optimizer="adamw", eval_every=0, test_samples=16, **HP),
                        log=lambda *a, **k: None)["server"]
    finally:
        torch.set_num_threads(nt)
    assert srv["optimizer"] == "adamw" and srv["adamw"]["steps"] == srv["global_steps_completed"]
    assert srv["global_steps_completed"] == loc["global_steps_completed"] > 0
    assert srv["final_param_checksum"] == pytest.approx(loc["final_param_checksum"], rel=1e-6)
