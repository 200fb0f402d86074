"""--optimizer muon on the CPU path: configuration scope, the rule's host form against an fp64
reference written here (shared with the GPU tests), partial ranges, metrics, checkpoint / resume."""
import numpy as np
import pytest
import torch

from psx.models.layout import Entry, ParamLayout
from psx.parallel import rules as R
from psx.parallel.server import ParameterServer
from psx.utils.config import parse

from .test_lamb_cpu import tiny_server
from .test_ps_cpu import tiny_cfg

COEF = (3.4445, -4.7750, 2.0315)


def ns_chain(U, steps=5, coef=COEF, normalize=True, dtype=torch.float64):
    """The chain on one matrix in plain torch ``dtype``: (O in U's orientation, max |intermediate|)."""
    a, b, c = coef
    X = U.to(dtype)
    if normalize:
        X = X / (X.norm() + 1e-7)
    tall = U.shape[0] > U.shape[1]
    X = X.t() if tall else X
    big = 0.0
    for _ in range(steps):
        A = X @ X.t()
        AA = A @ A
        B = b * A + c * AA
        BX = B @ X
        X = a * X + BX
        big = max([big] + [float(t.abs().max()) for t in (A, AA, B, BX, X)])
    return (X.t() if tall else X), big


def chain_yardstick(mats) -> float:
    """The tolerance's unit: the torch fp32 CPU chain's largest error against the fp64 chain."""
    return max(float((ns_chain(U, dtype=torch.float32)[0].double() - ns_chain(U)[0]).abs().max()) for U in mats)


def synthetic_layout():
    """Two convs (one of two chunks, one whose K is split in slabs), a tall 1x1, BN, FC."""
    lay, off = ParamLayout(), 0
    for name, shape in (("conv1.weight", (32, 40, 3, 3)), ("bn1.weight", (13,)), ("bn1.bias", (13,)),
                        ("conv2.weight", (8, 89, 3, 3)), ("short.weight", (40, 16, 1, 1)), ("fc.weight", (10, 40)),
                        ("fc.bias", (10,))):
        n = int(np.prod(shape))
        lay.entries[name] = Entry(name, shape, "float32", "param", off, n)
        off += n
    lay.param_numel = off
    return lay


def matrices(lay, flat):
    return [flat[e.offset:e.offset + e.numel].view(e.shape[0], -1) for e in lay.entries.values() if len(e.shape) > 1]


def muon_reference(lay, p, buf, s, lr, aux_lr, gscale, mu, wd, steps=5):
    """One Muon update in fp64 from fp32 p, buf (None with mu = 0) and the fp32 wire sum s:
    (p', buf', u, lr_of) with lr_of the per-element factor on O (0 on 1-D tensors). buf' is within
    2^-22 (|mu buf| + |g|) of the fp32 forms: two roundings relative to the magnitudes summed."""
    f = lambda x: float(np.float32(x))
    g = f(gscale) * s.double()
    b2 = f(mu) * buf.double() + g if buf is not None else None
    u = g + f(mu) * b2 if buf is not None else g
    p2, lr_of = p.double().clone(), torch.zeros_like(g)
    for e in lay.entries.values():
        sl = slice(e.offset, e.offset + e.numel)
        if len(e.shape) > 1:
            rows, cols = e.shape[0], e.numel // e.shape[0]
            O, _ = ns_chain(u[sl].view(rows, cols), steps)
            lr_of[sl] = f(lr) * max(1.0, rows / cols) ** 0.5
            p2[sl] = p2[sl] * (1.0 - f(lr) * f(wd)) - lr_of[sl] * O.reshape(-1)
        else:
            p2[sl] -= f(aux_lr or lr) * u[sl]
    return p2, b2, u, lr_of


def buf_bound(b_old, s, gscale, mu):
    return 2.0 ** -22 * (float(np.float32(mu)) * b_old.double().abs() + float(np.float32(gscale)) * s.double().abs())


def update_bound(lay, u, lr_of, p_ref, p_old):
    """4 x the chain yardstick on this update's own matrices, times the factor on O. The issue's
    bound stops there; but w is stored in fp32 and 1-D tensors have no chain term, so the fp32
    roundings outside the chain are added: 2^-23 |w| (two: the decay product, the final sum) and
    2^-22 |step| (up to four: u's two, lr * sqrt(rows / cols), the product with O or u)."""
    yard = chain_yardstick(matrices(lay, u.float()))
    return 4 * yard * lr_of + 2.0 ** -23 * p_old.double().abs() + 2.0 ** -22 * (p_ref - p_old.double()).abs()


# ---------------------------------------------------------------------------- configuration
def test_config_scope():
    cfg = parse(["--optimizer", "muon", "--momentum", "0.95", "--muon-ns-steps", "3", "--muon-aux-lr", "0.05"])
    assert (cfg.optimizer, cfg.momentum, cfg.muon_ns_steps, cfg.muon_aux_lr) == ("muon", 0.95, 3, 0.05)
    d = parse(["--optimizer", "muon"])
    assert (d.muon_ns_steps, d.muon_aux_lr, d.momentum) == (5, 0.0, 0.0)
    assert type(R.rule_of(d)) is R.Muon and d.whole_arena_update and d.resolve_overlap(8) is False
    for bad in (["--topology", "sharded"], ["--overlap"], ["--mode", "async", "--dc-lambda", "0.04"],
                ["--clip-norm", "1.0"], ["--muon-ns-steps", "0"]):
        with pytest.raises(ValueError, match="--optimizer muon"):
            parse(["--optimizer", "muon"] + bad)


# ---------------------------------------------------------------------------- server numerics
def synthetic_server(device="cpu", **kw):
    lay = synthetic_layout()
    arena = torch.randn(lay.param_numel, generator=torch.Generator().manual_seed(1)) * 0.1
    cfg = tiny_cfg(**{**dict(mode="sync", workers=2, optimizer="muon", lr=0.02, momentum=0.95, weight_decay=0.01,
                             muon_aux_lr=0.05, codec="none"), **kw})
    s = ParameterServer(cfg, lay, arena, None, device=device, total_workers=cfg.workers, log=lambda *a: None)
    for w in range(cfg.workers):
        s.register_worker("w", w)
    return s, lay, cfg


@pytest.mark.parametrize("mu", [0.0, 0.95])
def test_host_form_matches_reference(mu):
    """Two rounds of two fp32 wires on a CPU arena against the fp64 formula, each round from the
    server's own state before it."""
    s, lay, cfg = synthetic_server(momentum=mu)
    assert (s.momentum_buf is None) == (mu == 0.0)
    with pytest.raises(ValueError, match="--optimizer muon"):  # a partial range
        s.apply_range(torch.zeros(8), 1.0, 0, 8)
    gen = torch.Generator().manual_seed(5)
    for rnd in range(2):
        srcs = [torch.randn(lay.param_numel, generator=gen) * 1e-2 for _ in range(2)]
        p_old, b_old = s.params.clone(), s.momentum_buf.clone() if mu else None
        p_ref, b_ref, u, lr_of = muon_reference(lay, p_old, s.momentum_buf, srcs[0] + srcs[1], cfg.lr, cfg.muon_aux_lr,
                                                0.5, mu, cfg.weight_decay)
        assert s.apply_sources(srcs, [0, 1], [rnd + 1] * 2)
        err = (s.params.double() - p_ref).abs()
        assert bool((err <= update_bound(lay, u, lr_of, p_ref, p_old)).all()), (rnd, float(err.max()))
        if mu:
            assert bool(((s.momentum_buf.double() - b_ref).abs() <= buf_bound(b_old, srcs[0] + srcs[1], 0.5, mu)).all())
    norms = [float(U.norm()) for U in matrices(lay, u)]
    assert s._muon_norms == pytest.approx(norms, rel=1e-5)
    fm = s.final_metrics()
    assert fm["optimizer"] == "muon" and fm["muon"] == {"ns_steps": 5, "momentum": mu, "aux_lr": 0.05}
    assert fm["muon_update_norm"]["max"] == pytest.approx(max(norms), rel=1e-5)


def test_checkpoint_resume(tmp_path):
    """The momentum buffer travels with the checkpoint: the resumed run continues bit for bit."""
    kw = dict(optimizer="muon", momentum=0.95, codec="none", ckpt_dir=str(tmp_path), lr=0.02)
    a, lay, _ = tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2, g3 = (torch.randn(lay.param_numel, generator=gen) * 1e-2 for _ in range(3))
    a.apply(g1, 1.0)
    path = a.checkpoint()
    a.apply(g2, 1.0)
    a.apply(g3, 1.0)
    b, _, _ = tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 1 and bool(b.momentum_buf.any())
    b.apply(g2, 1.0)
    b.apply(g3, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.momentum_buf, b.momentum_buf)
