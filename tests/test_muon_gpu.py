"""csrc/kernels/muon.hip through K.muon_orthogonalize and K.muon_apply_multi against the plain fp64
references of tests/test_muon_cpu.py: the grouped chain, and the whole update on a small layout."""
import itertools

import pytest
import torch

from psx.ops import kernels as K

from .test_muon_cpu import buf_bound, muon_reference, ns_chain, synthetic_layout, update_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
# one table: tall with an odd K, m no multiple of 16, a tall 1x1, a wide 3x3, > 2 tiles each way
# and 8 x 801: K split in two slabs, or with a slab cap of 8 in 9, 9 and 8 K tiles (a short last slab)
SHAPES = [(16, 16), (64, 27), (100, 512), (128, 64), (64, 576), (144, 200), (8, 801)]


@pytest.mark.parametrize("cap", [2, 8])
def test_chain_is_exact_on_small_integers(cap, monkeypatch):
    """One iteration, coef (1, 1, 1), no normalisation, entries in {-1, 0, 1}: every intermediate
    is an integer below 2^24, so any summation order gives the fp64 result's bits. A wrong tile
    index, mirror write, transpose, slab or pad shows here."""
    monkeypatch.setenv("PSX_TUNE", f"mu_slabs={cap}")
    gen = torch.Generator().manual_seed(0)
    mats = []
    for r, c in SHAPES:
        u = torch.rand(r, c, generator=gen)
        mats.append((u > 7 / 8).float() - (u < 1 / 8).float())
    refs = [ns_chain(U, 1, (1.0, 1.0, 1.0), normalize=False) for U in mats]
    assert max(big for _, big in refs) < 2 ** 24
    outs = K.muon_orthogonalize([U.to(DEV) for U in mats], steps=1, coef=(1.0, 1.0, 1.0), normalize=False)
    for shape, out, (ref, _) in zip(SHAPES, outs, refs):
        assert out.shape == ref.shape and torch.equal(out.cpu().double(), ref), shape


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_five_step_chain(seed):
    """randn inputs, five steps with the Muon coefficients: per shape, the kernel's max-abs error
    against the fp64 chain is at most 4 x that of the torch fp32 CPU chain on the same inputs (the
    margin is for the other summation order, and the norm folded into the first iteration).
    Measured on an MI355X: err / yardstick between 0.67 and 1.41 over these shapes and seeds."""
    gen = torch.Generator().manual_seed(seed)
    mats = [torch.randn(r, c, generator=gen) for r, c in SHAPES]
    outs = K.muon_orthogonalize([U.to(DEV) for U in mats])
    for shape, U, out in zip(SHAPES, mats, outs):
        ref = ns_chain(U)[0]
        yard = float((ns_chain(U, dtype=torch.float32)[0].double() - ref).abs().max())
        err = float((out.cpu().double() - ref).abs().max())
        print(f"muon chain {shape} seed {seed}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        assert err <= 4 * yard, (shape, err, yard)


def _update(W, half, mu, wd, image, aux, rounds=2):
    """``rounds`` updates, each against the fp64 reference from the device's state before it."""
    lay = synthetic_layout()
    n = lay.param_numel
    gen = torch.Generator().manual_seed(7)
    p = (torch.randn(n, generator=gen) * 0.1).to(DEV)
    buf = torch.zeros(n, device=DEV) if mu else None
    img = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if image else None
    stage = torch.empty(n, device=DEV)
    tab = K.lars_table(lay, DEV)
    mtab = K.MuonTable(lay, DEV, tab)
    lr, gscale = 0.02, 1.0 / W
    for _ in range(rounds):
        srcs = [torch.randn(n, generator=gen) * 1e-2 for _ in range(W)]
        srcs = [s.half() if half else s for s in srcs]
        ssum = torch.zeros(n)
        for s in srcs:
            ssum = ssum + s.float()
        p_old, b_old = p.cpu(), buf.cpu() if mu else None
        p_ref, b_ref, u, lr_of = muon_reference(lay, p_old, b_old, ssum, lr, aux, gscale, mu, wd)
        K.muon_apply_multi(p, [s.to(DEV) for s in srcs], stage, buf, tab, mtab, lr, aux_lr=aux, gscale=gscale,
                           momentum=mu, wd=wd, img=img)
        torch.cuda.synchronize()
        assert torch.equal(stage.cpu(), ssum)
        err = (p.cpu().double() - p_ref).abs()
        tol = update_bound(lay, u, lr_of, p_ref, p_old)
        assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())
        if mu:
            assert bool(((buf.cpu().double() - b_ref).abs() <= buf_bound(b_old, ssum, gscale, mu)).all())
        if image:
            assert torch.equal(img, p.bfloat16())
        norms = torch.tensor([float(u[e.offset:e.offset + e.numel].norm()) for e in lay.entries.values()
                              if len(e.shape) > 1])
        assert torch.allclose(tab.ratios.cpu()[torch.tensor(tab.adapt)].double(), norms.double(), rtol=1e-5)
    return p, buf, img


@pytest.mark.parametrize("W,half,mu,wd,image,aux", list(itertools.product((1, 3), (True, False), (0.0, 0.95),
                                                                          (0.0, 0.01), (True, False), (0.0, 0.05))))
def test_whole_update(W, half, mu, wd, image, aux):
    """Two updates in a row (so the momentum buffer matters) against the fp64 reference of the
    rule; the bf16 image is the rounding of the fp32 parameters the kernel wrote."""
    _update(W, half, mu, wd, image, aux)


def test_two_runs_give_the_same_bits():
    a, b = _update(3, True, 0.95, 0.01, True, 0.05), _update(3, True, 0.95, 0.01, True, 0.05)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
