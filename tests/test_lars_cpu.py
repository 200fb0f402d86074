"""--optimizer lars on the CPU path: configuration scope, the torch implementation of the update
in ParameterServer against an fp64 reference written here from the formula, and checkpoint /
resume. The reference (lars_reference) is shared with the GPU kernel tests."""
import json
import types

import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel import q8 as Q
from psx.parallel import topk as T
from psx.parallel.server import ParameterServer
from psx.utils import checkpoint as ckpt
from psx.utils.config import PSConfig

from .test_ps_cpu import tiny_cfg


def f32(x) -> float:
    """A hyper-parameter as the kernels' C ABI receives it (a float)."""
    return float(np.float32(x))


def lars_reference(layout, p, s, v, *, lr, gscale, momentum, wd, trust, eps, first, f32_hparams=False):
    """The update of one round in fp64, straight from the definition. ``s``: the fp32 sum of the
    decoded worker gradients (the reference starts from the same fp32 s as the code under test);
    ``p``, ``v``: parameters and momentum buffer before the update (v None or unused without
    momentum). Returns (p_new, v_new or None, {tensor name: lambda_t}) in fp64."""
    if f32_hparams:
        lr, gscale, momentum, wd, trust, eps = (f32(x) for x in (lr, gscale, momentum, wd, trust, eps))
    p = p.double().clone()
    g = gscale * s.double()
    v_new = torch.zeros_like(p) if momentum else None
    ratios = {}
    for e in layout.entries.values():
        if e.region != "param":
            continue
        sl = slice(e.offset, e.offset + e.numel)
        w, gt = p[sl], g[sl]
        if len(e.shape) > 1:
            wn, gn = float(w.square().sum().sqrt()), float(gt.square().sum().sqrt())
            lam = trust * wn / (gn + wd * wn + eps) if wn > 0 and gn > 0 else 1.0
            d = lam * (gt + wd * w)
        else:
            lam, d = 1.0, gt
        ratios[e.name] = lam
        if momentum:
            d = d if first else momentum * v[sl].double() + d
            v_new[sl] = d
        p[sl] = w - lr * d
    return p, v_new, ratios


def assert_update_close(p_new, p_old, p_ref, what=""):
    """|delta - delta_ref| <= 2e-5 |delta_ref| + 2^-23 |p_old| (the second term: the rounding of
    the final subtraction)."""
    d, d_ref = p_new.double() - p_old.double(), p_ref - p_old.double()
    err, tol = (d - d_ref).abs(), 2e-5 * d_ref.abs() + 2.0 ** -23 * p_old.double().abs()
    bad = err > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - tol).max()))


def assert_buf_close(v_new, v_ref, what=""):
    err, tol = (v_new.double() - v_ref).abs(), 2e-5 * v_ref.abs()
    bad = err > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / v_ref.abs().clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------- configuration
def test_config_scope():
    cfg = PSConfig(optimizer="lars").validate()
    assert cfg.lars_trust == 0.001 and cfg.lars_eps == 1e-8
    assert PSConfig().validate().optimizer == "sgd"
    with pytest.raises(ValueError):
        PSConfig(optimizer="adam").validate()
    with pytest.raises(ValueError, match="--optimizer lars"):
        PSConfig(optimizer="lars", topology="sharded", mode="sync").validate()
    with pytest.raises(ValueError, match="--optimizer lars"):
        PSConfig(optimizer="lars", overlap=True).validate()
    with pytest.raises(ValueError):
        PSConfig(optimizer="lars", lars_trust=0.0).validate()
    assert PSConfig(mode="sync", optimizer="lars").validate().resolve_overlap(8) is False
    assert PSConfig(mode="sync").validate().resolve_overlap(8) is True


def test_cli_flags():
    from psx.utils.config import parse

    cfg = parse(["--optimizer", "lars", "--lars-trust", "0.02", "--lars-eps", "1e-6", "--momentum", "0.9",
                 "--weight-decay", "5e-4"])
    assert (cfg.optimizer, cfg.lars_trust, cfg.lars_eps, cfg.momentum, cfg.weight_decay) == \
        ("lars", 0.02, 1e-6, 0.9, 5e-4)
    assert parse([]).optimizer == "sgd"


def test_native_paths_decline_lars(monkeypatch):
    """The paths that apply per bucket or inside native C++ loops fall back to the Python server
    (or refuse) under LARS; with SGD the same stubs select them."""
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
    for opt, want in (("sgd", True), ("lars", False)):
        a = PSConfig(mode="async", optimizer=opt).validate()
        assert native_loop_enabled(a, t) is want
        s = PSConfig(mode="sync", topology="dedicated", optimizer=opt).validate()
        chan = SyncCollectiveChannel(t, srv, members=[0, 1], codec=None, root_worker=False)
        assert native_sync_enabled(s, t, chan, srv, 0) is want
        c = PSConfig(mode="sync", topology="colocated", optimizer=opt).validate()
        assert graph_round_enabled(c, t) is want
    lars = PSConfig(mode="async", optimizer="lars").validate()
    stub = types.SimpleNamespace(cfg=lars, layout=None, device="cpu")
    with pytest.raises(ValueError, match="--optimizer lars"):
        NativeServerLoop(stub, None, None, {}, 1)
    with pytest.raises(ValueError, match="--optimizer lars"):
        NativeSyncServer(stub, t, None)
    with pytest.raises(ValueError, match="--optimizer lars"):
        run_local_threads(lars, 1)


# ---------------------------------------------------------------------------- server numerics
def _tiny_server(**kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(mode="async", workers=1, optimizer="lars", **kw)
    s = ParameterServer(cfg, lay, arena.clone(), counters, total_workers=1, log=lambda *a: None)
    s.register_worker("w", 0)
    return s, lay, cfg


def _wires(kind: str, n: int, steps: int, cfg, sign: torch.Tensor):
    """``steps`` pushes of one wire kind with the dense fp32 gradient each decodes to. Every
    gradient element carries ``sign`` (the sign of its weight): the tolerances of these tests are
    relative to the result, which a sum has to earn by not cancelling — with one sign per element
    g + wd * w and momentum * v + d add magnitudes. The encoders start each push without residual,
    so a decoded element keeps its sign or is zero."""
    gen = torch.Generator().manual_seed(11)
    out = []
    enc = Q.Q8Codec(n) if kind == "q8" else T.TopKCodec(n, cfg.topk_ratio, "cpu") if kind == "topk" else None
    for _ in range(steps):
        g = sign * torch.randn(n, generator=gen).abs() * 1e-2
        if enc is not None:
            enc.resid.zero_()
        if kind == "fp16":
            wire = g.half()
            dense = wire.float()
        elif kind == "q8":
            wire = enc.encode(g).clone()
            dense = Q.decode(wire, n)
        else:
            wire = enc.encode(g).clone()
            dense = T.decode_add(wire, torch.zeros(n), 1.0, T.topk_k(n, cfg.topk_ratio)).clone()
        out.append((wire, dense))
    return out


@pytest.mark.parametrize("kind", ["fp16", "q8", "topk"])
def test_server_apply_matches_reference(kind):
    """ParameterServer.apply on a CPU arena, two consecutive pushes (first-step and running
    momentum), against the fp64 reference applied to the decoded gradient."""
    codec = {"fp16": "fp16", "q8": "q8", "topk": "topk"}[kind]
    s, lay, cfg = _tiny_server(codec=codec, momentum=0.9, weight_decay=5e-4, lr=0.1, topk_ratio=0.25)
    n = lay.param_numel
    kw = dict(lr=cfg.lr, gscale=1.0, momentum=cfg.momentum, wd=cfg.weight_decay, trust=cfg.lars_trust,
              eps=cfg.lars_eps)
    sign = torch.where(s.params >= 0, 1.0, -1.0)
    for step, (wire, dense) in enumerate(_wires(kind, n, 2, cfg, sign)):
        assert bool((dense * sign >= 0).all())
        p_old, v_old = s.params.clone(), s.momentum_buf.clone()
        p_ref, v_ref, ratios = lars_reference(lay, p_old, dense, v_old, first=step == 0, **kw)
        s.apply(wire, 1.0)
        assert_update_close(s.params, p_old, p_ref, (kind, step))
        assert_buf_close(s.momentum_buf, v_ref, (kind, step))
        got = s.lars_trust_ratios()
        adapted = torch.tensor([ratios[e.name] for e in lay.entries.values()
                                if e.region == "param" and len(e.shape) > 1])
        for key, want in (("min", adapted.min()), ("median", adapted.median()), ("max", adapted.max())):
            assert got[key] == pytest.approx(float(want), rel=1e-5)
    assert s.core.global_step == 2
    m = s.final_metrics()
    assert m["optimizer"] == "lars" and set(m["lars_trust_ratio"]) == {"min", "median", "max"}
    assert 0 < m["lars_trust_ratio"]["min"] <= m["lars_trust_ratio"]["median"] <= m["lars_trust_ratio"]["max"]


def test_one_dim_tensors_take_plain_sgd_without_decay():
    """BN affine parameters and the FC bias: lambda = 1 and no weight decay, i.e. exactly the SGD
    server's update with wd = 0; tensors with ndim > 1 move differently."""
    s, lay, cfg = _tiny_server(codec="none", momentum=0.9, weight_decay=5e-4, lr=0.1)
    sgd_cfg = tiny_cfg(mode="async", workers=1, codec="none", momentum=0.9, weight_decay=0.0, lr=0.1)
    r = ParameterServer(sgd_cfg, lay, s.arena.clone(), s.counters, total_workers=1, log=lambda *a: None)
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        g = torch.randn(lay.param_numel, generator=gen) * 1e-2
        s.apply(g, 0.5)
        r.apply(g, 0.5)
    for e in lay.entries.values():
        if e.region != "param":
            continue
        a, b = lay.view(s.arena, e.name), lay.view(r.arena, e.name)
        assert torch.equal(a, b) == (len(e.shape) == 1), e.name


def test_partial_range_raises():
    s, lay, _ = _tiny_server(codec="none")
    n = lay.param_numel
    g = torch.zeros(n)
    with pytest.raises(ValueError, match="--optimizer lars"):
        s.apply_range(g[: n // 2], 1.0, 0, n // 2)
    with pytest.raises(ValueError, match="--optimizer lars"):
        s.apply_range_sources([g], 1.0, 8, n)


def test_sgd_metrics_name_the_optimizer():
    cfg = tiny_cfg(mode="async", workers=1)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    s = ParameterServer(cfg, lay, arena, counters, total_workers=1, log=lambda *a: None)
    fm = s.final_metrics()
    assert fm["optimizer"] == "sgd" and "lars_trust_ratio" not in fm


def test_run_local_sync_lars():
    from psx.parallel.runner import run_local

    cfg = tiny_cfg(mode="sync", workers=2, optimizer="lars", momentum=0.9, weight_decay=5e-4, eval_every=0)
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    assert srv["optimizer"] == "lars" and srv["global_steps_completed"] > 0
    assert srv["lars_trust_ratio"]["max"] > 0 and srv["final_param_checksum"] == srv["final_param_checksum"]


# ---------------------------------------------------------------------------- checkpoint / resume
def test_checkpoint_resume(tmp_path):
    """Checkpoint after one update, resume into a fresh server, apply the same second gradient:
    the arenas are equal (LARS keeps no state besides the momentum buffer)."""
    kw = dict(codec="none", momentum=0.9, weight_decay=5e-4, lr=0.1, ckpt_dir=str(tmp_path))
    a, lay, _ = _tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2 = (torch.randn(lay.param_numel, generator=gen) * 1e-2 for _ in range(2))
    a.apply(g1, 1.0)
    path = a.checkpoint()
    a.apply(g2, 1.0)
    b, _, _ = _tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 1 and not b._mom_first
    b.apply(g2, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.momentum_buf, b.momentum_buf)
    saved = json.loads(ckpt.load(path)["config"])  # the optimizer travels in the checkpoint's config
    assert saved["optimizer"] == "lars" and saved["lars_trust"] == 0.001
