"""The merged backward transform of the three-launch Winograd layers (csrc/kernels/wino.hip
wino_dz_xf_kernel): one pass over dz writes V' = B^T dy B (the data gradient's operand) and
D = A dy A^T (the weight gradient's), optionally with the BN-backward apply folded into the load.

The fold has two roundings of dy: the other folded consumers' (wino_bwd_apply, the default of the
entry) and, as_apply, the apply pass's own, which the engine runs so that its step stays bit-equal
to the unfolded one. Plain: V' is bit-equal to the V wino_conv leaves for the same input and D to the D wino_wgrad
leaves in its scratch. Fold: D is bit-equal to wino_wgrad(..., bwd_in=fold)'s, V' is held to a
float64 B^T (k1 dz + k2 y + k3) B built from the published coefficients (padding zeroed after the
fold) under test_wino_gpu.py's bar (max-abs error <= 1e-4 of the reference's max-abs), and the
published coefficients, dgamma and dbeta are bit-equal to bn_bwd_apply_fin's for the same slot
sums, on the fp32 and the fp16 wire. wino_wgrad refuses tile counts that are no multiple of 32
(its GEMM's), so where a shape has one its D reference comes from the same images at the front of
a batch padded to the next such count: tile t's D does not depend on the other tiles, and the
fold's coefficients come from the slot sums and the descriptor's count, not from the batch.
Every buffer sits between canaries, the outputs start as NaN; every case runs with deterministic
mode on and off (the fold reads the slot rows in either format). Engine level (ResNet-18): the
new path against PSX_TUNE=wino_bwdfold=0, the side-stream engine staying on the old launches,
and bit-reproducibility in deterministic mode."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from psx.ops import kernels as K  # noqa: E402

from .test_sgd_gpu import DEV, Placed, bits  # noqa: E402
from .test_wino_gpu import TOL, _rel  # noqa: E402

NAN = float("nan")
# nb, h, w, k
SHAPES = [(2, 4, 4, 64),     # T = 2: fewer tiles than grid rows; every window row / column 0 and 5 is padding
          (8, 8, 8, 128),    # two channel blocks, interior tile edges
          (3, 7, 7, 64),     # partial edge tiles, both directions
          (3, 6, 10, 64),    # partial edge tiles, h != w
          (80, 8, 8, 512)]   # T = 320 over 128 grid rows: 3 or 2 iterations per workgroup (the buffers wrap)
IDS = ["%dx%dx%dx%d" % s for s in SHAPES]


@pytest.fixture(params=[False, True], ids=["atomic", "det"])
def det(request):
    K.set_deterministic(request.param)
    yield request.param
    K.set_deterministic(None)


def _tiles(nb, h, w):
    return nb * ((h + 3) // 4) * ((w + 3) // 4)


def _nb_pad(nb, h, w):
    """The smallest batch >= nb whose tile count is a multiple of 32 (what wino_wgrad takes)."""
    tpi = _tiles(1, h, w)
    step = 32 // math.gcd(32, tpi)
    return -(-nb // step) * step


def _nan(n):
    return torch.full((n,), NAN, device=DEV)


def _case(nb, h, w, k, seed):
    """dz and y of the padded batch (the test's images in front), the BN's saved statistics and gamma."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nbp = _nb_pad(nb, h, w)
    dz = torch.randn(nbp, h, w, k, device=DEV, generator=g)
    y = torch.randn(nbp, h, w, k, device=DEV, generator=g) * 1.5 + 0.3
    saved = torch.stack([torch.randn(k, device=DEV, generator=g) * 0.2 + 0.3,
                         torch.rand(k, device=DEV, generator=g) * 0.5 + 0.5]).contiguous()
    gamma = torch.rand(k, device=DEV, generator=g) + 0.5
    return nbp, dz, y, saved, gamma


def _slot_sums(dz, y, saved, k):
    """The BN-backward slot rows of dz (row 0 sum dz, row 1 sum dz xhat) in the current mode's format."""
    part = torch.zeros(K.STAT_SLOTS * (K.det_slot_scale() if K.deterministic() else 1), 2, k, device=DEV)
    K.bn_bwd_reduce(dz, torch.ones_like(dz), y, saved, part, dz.numel() // k, k)
    return part


class Fin:
    """A BnBwdFin with its own coefficient / dgamma / dbeta buffers (NaN until a launch publishes them)."""

    def __init__(self, gamma, saved, count, k, fp16, gscale):
        self.coef = Placed(_nan(3 * k))
        self.dgb = Placed(torch.full((2 * k,), NAN, device=DEV, dtype=torch.float16 if fp16 else torch.float32))
        self.ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
        p = self.dgb.view.data_ptr()
        self.fin = K.bn_bwd_fin(gamma, saved, self.coef.view, p, p + k * self.dgb.view.element_size(),
                                self.ctr.data_ptr(), count, gscale, k, fp16)


def _dz_xf(dz, nb, h, w, k, bwd_in=None, as_apply=False):
    n = K.wino_v_floats(nb, h, w, k)
    src, v, d = Placed(dz.reshape(-1)), Placed(_nan(n)), Placed(_nan(n))
    ybn = Placed(bwd_in[0].reshape(-1)) if bwd_in is not None else None
    rc = K.wino_dz_xf(src.view, v.view, d.view, nb, h, w, k,
                      bwd_in=(ybn.view,) + tuple(bwd_in[1:]) if bwd_in is not None else None, as_apply=as_apply)
    torch.cuda.synchronize()
    assert rc == 0
    for p in (src, v, d) + ((ybn,) if ybn is not None else ()):
        assert p.intact(), "canary overwritten"
    assert src.unchanged() and (ybn is None or ybn.unchanged())
    assert not bool(torch.isnan(v.view).any()) and not bool(torch.isnan(d.view).any()), "an element was not written"
    T = _tiles(nb, h, w)
    return v.view.view(36, T, k), d.view.view(36, T, k)


def _conv_v(x, nb, h, w, c):
    """The V wino_conv leaves for x (weights zero: only its input transform matters here)."""
    u = torch.zeros(36 * 64 * c, device=DEV)
    v = _nan(K.wino_v_floats(nb, h, w, c))
    p = torch.empty(K.wino_p_floats(nb, h, w, c, 64), device=DEV)
    K.wino_conv(x, u, torch.empty(nb, h, w, 64, device=DEV), None, None, v, p, nb, h, w, c, 64)
    torch.cuda.synchronize()
    return v.view(36, _tiles(nb, h, w), c)


def _wgrad_d(dy, nbp, h, w, k, bwd_in=None):
    """The D wino_wgrad leaves in its scratch for the (padded) batch dy."""
    c = 64
    q = K.wino_wgrad_q(nbp, h, w, c, k)
    assert q > 0
    v = torch.zeros(K.wino_v_floats(nbp, h, w, c), device=DEV)
    d = _nan(K.wino_v_floats(nbp, h, w, k))
    K.wino_wgrad(v, dy, d, torch.empty(36 * q * k * c, device=DEV), torch.empty(k * c * 9, device=DEV), nbp, h, w, c, k,
                 bwd_in=bwd_in)
    torch.cuda.synchronize()
    return d.view(36, _tiles(nbp, h, w), k)


def _same_bits(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


@pytest.mark.parametrize("nb,h,w,k", SHAPES, ids=IDS)
def test_plain_bit_equal_to_the_two_transforms(nb, h, w, k, det):
    nbp, dzp, _, _, _ = _case(nb, h, w, k, seed=nb + h + k)
    dz = dzp[:nb].contiguous()
    v, d = _dz_xf(dz, nb, h, w, k)
    T = _tiles(nb, h, w)
    assert _same_bits(v, _conv_v(dz, nb, h, w, k))
    assert _same_bits(d, _wgrad_d(dzp, nbp, h, w, k)[:, :T])


BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
      [0, 4, 0, -5, 0, 1]]


def _v_ref64(dy, nb, h, w, k):
    """B^T d B in float64 of every 6x6 window (at (4 ti - 1, 4 tj - 1), zero padded) of dy [nb][h][w][k]."""
    th, tw = (h + 3) // 4, (w + 3) // 4
    pad = torch.zeros(nb, 4 * th + 2, 4 * tw + 2, k, dtype=torch.float64, device=DEV)
    pad[:, 1:h + 1, 1:w + 1] = dy
    win = pad.unfold(1, 6, 4).unfold(2, 6, 4)  # [nb][th][tw][k][6][6]
    bt = torch.tensor(BT, dtype=torch.float64, device=DEV)
    v = torch.einsum("ar,nijkrs,bs->abnijk", bt, win, bt)
    return v.reshape(36, nb * th * tw, k)


@pytest.mark.parametrize("fp16", [False, True], ids=["wire32", "wire16"])
@pytest.mark.parametrize("nb,h,w,k", SHAPES, ids=IDS)
def test_fold(nb, h, w, k, fp16, det):
    nbp, dzp, yp, saved, gamma = _case(nb, h, w, k, seed=nb + h + k + 1)
    dz, y = dzp[:nb].contiguous(), yp[:nb].contiguous()
    cnt = nb * h * w
    part = _slot_sums(dz, y, saved, k)
    gscale = 1.0 / 3
    got, ref, ign = (Fin(gamma, saved, cnt, k, fp16, gscale) for _ in range(3))
    v, d = _dz_xf(dz, nb, h, w, k, bwd_in=(y, part, got.fin))
    # the coefficients and dgamma / dbeta: what bn_bwd_apply_fin writes for the same slot sums
    K.bn_bwd_apply_fin(dz, None, y, part, ref.fin, torch.empty_like(dz), k)
    torch.cuda.synchronize()
    assert got.coef.intact() and got.dgb.intact()
    assert _same_bits(got.coef.view, ref.coef.view)
    assert _same_bits(got.dgb.view, ref.dgb.view)
    assert not bool(torch.isnan(got.dgb.view.float()).any())
    # D: wino_wgrad's folded dy transform (it publishes nothing)
    T = _tiles(nb, h, w)
    assert _same_bits(d, _wgrad_d(dzp, nbp, h, w, k, bwd_in=(yp, part, ign.fin))[:, :T])
    assert bool(torch.isnan(ign.coef.view).all())
    # V': float64 from the published coefficients, padding zeroed after the fold
    k1, k2, k3 = got.coef.view.view(3, k).double()
    err = _rel(v, _v_ref64(k1 * dz.double() + k2 * y.double() + k3, nb, h, w, k))
    print(f"fold V' vs fp64: {err:.2e} (bar {TOL:.0e})")
    assert err < TOL


@pytest.mark.parametrize("nb,h,w,k", SHAPES, ids=IDS)
def test_fold_as_apply_is_the_transform_of_the_written_dy(nb, h, w, k, det):
    """The fold the engine runs (as_apply: dy rounded as bn_bwd_apply_fin writes it): V' and D are
    bit for bit the plain transforms of the dy that pass writes for the same slot sums, and the
    published coefficients and dgamma / dbeta are its own — a step that folds equals one that does not."""
    _, dzp, yp, saved, gamma = _case(nb, h, w, k, seed=nb + h + k + 2)
    dz, y = dzp[:nb].contiguous(), yp[:nb].contiguous()
    cnt = nb * h * w
    part = _slot_sums(dz, y, saved, k)
    got, ref = (Fin(gamma, saved, cnt, k, True, 0.5) for _ in range(2))
    dy = torch.full_like(dz, NAN)
    K.bn_bwd_apply_fin(dz, None, y, part, ref.fin, dy, k)
    torch.cuda.synchronize()
    v, d = _dz_xf(dz, nb, h, w, k, bwd_in=(y, part, got.fin), as_apply=True)
    v0, d0 = _dz_xf(dy, nb, h, w, k)
    assert _same_bits(v, v0) and _same_bits(d, d0)
    assert _same_bits(got.coef.view, ref.coef.view) and _same_bits(got.dgb.view, ref.dgb.view)


def test_host_refusals():
    """-2 (not this shape) and -3 (inconsistent fold arguments) come back before any launch: the
    outputs stay NaN."""
    k = 64
    dz, y = torch.randn(2, 4, 4, k, device=DEV), torch.randn(2, 4, 4, k, device=DEV)
    v, d = _nan(K.wino_v_floats(2, 4, 4, k)), _nan(K.wino_v_floats(2, 4, 4, k))
    f = Fin(torch.ones(k, device=DEV), torch.ones(2, k, device=DEV), 32, k, False, 1.0)
    part = torch.zeros(K.STAT_SLOTS * K.det_slot_scale(), 2, k, device=DEV)
    lib = K.kernels()
    from psx.ops._lib import stream_ptr
    import ctypes as C

    def call(h, w, kk, ybn, bpart, fin):
        return lib.psx_wino_dz_xf(dz.data_ptr(), v.data_ptr(), d.data_ptr(), 2, h, w, kk,
                                  ybn.data_ptr() if ybn is not None else None,
                                  bpart.data_ptr() if bpart is not None else None,
                                  C.byref(fin) if fin is not None else None, stream_ptr())

    assert not K.wino_dz_ok(2, 2, 8, k) and not K.wino_dz_ok(2, 4, 4, 96) and not K.wino_dz_ok(2, 4, 4, 32)
    assert K.wino_dz_ok(2, 4, 4, k)
    assert call(2, 8, k, None, None, None) == -2     # an image side below 4
    assert call(4, 4, 96, None, None, None) == -2    # channels no power of two
    assert call(4, 4, 32, None, None, None) == -2    # fewer than 64 channels
    assert call(4, 4, k, None, part, f.fin) == -3    # slot sums without y
    assert call(4, 4, k, y, part, None) == -3        # ... without the descriptor
    assert call(4, 4, k, y, None, None) == -3        # y without slot sums
    wrong = Fin(torch.ones(128, device=DEV), torch.ones(2, 128, device=DEV), 32, 128, False, 1.0)
    assert call(4, 4, k, y, part, wrong.fin) == -3   # a descriptor of another channel count
    torch.cuda.synchronize()
    assert bool(torch.isnan(v).all()) and bool(torch.isnan(d).all()) and bool(torch.isnan(f.coef.view).all())


# ---- engine level: ResNet-18 ----

THREE_LAUNCH = {8: ["layer3.0.conv2", "layer3.1.conv1", "layer3.1.conv2"],
                32: ["layer3.0.conv2", "layer3.1.conv1", "layer3.1.conv2", "layer4.0.conv2", "layer4.1.conv1",
                     "layer4.1.conv2"]}


def _step(monkeypatch, tune, B, deterministic=True, **opts):
    """One eager step of a fresh engine under PSX_TUNE=``tune``; ``opts`` override fields of the
    EngineOptions that environment gives."""
    from dataclasses import replace

    from psx.models.engine import EngineOptions, HipResNetEngine
    from psx.models.layout import ParamLayout
    from psx.models.resnet import ResNet18

    torch.manual_seed(2)
    model = ResNet18(100)
    layout = ParamLayout.from_module(model)
    arena0, _ = layout.pack(model)
    arena0 = arena0.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    imgs = torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, device=DEV, generator=g)
    labs = torch.randint(0, 100, (64,), dtype=torch.int32, device=DEV, generator=g)
    if tune:
        monkeypatch.setenv("PSX_TUNE", tune)
    else:
        monkeypatch.delenv("PSX_TUNE", raising=False)
    options = replace(EngineOptions.from_env(True, (32, 32), deterministic), **opts)
    eng = HipResNetEngine(model, layout, B, dtype=torch.float32, options=options)
    eng.index.copy_(torch.arange(B, dtype=torch.int32, device=DEV))
    eng.train_step(arena0.clone(), imgs, labs)
    torch.cuda.synchronize()
    return eng, layout, [(eng.loss.double().mean().item(), eng.grads.clone())]


def _per_tensor(layout, g1, g0):
    errs = []
    for name, e in layout.entries.items():
        if e.region != "param":
            continue
        a, b = g1.double()[e.offset:e.offset + e.numel], g0.double()[e.offset:e.offset + e.numel]
        errs.append((((a - b).norm() / b.norm().clamp_min(1e-30)).item(), name))
    return sorted(errs)


@pytest.mark.parametrize("B,deterministic", [(8, True), (8, False), (32, True)], ids=["8-det", "8-atomic", "32-det"])
def test_engine_step_fold_vs_unfolded(B, deterministic, monkeypatch):
    """One step with the merged transform folding the BN-backward applies against
    PSX_TUNE=wino_bwdfold=0 (the merged transform without the fold): the forward is untouched, and
    every gradient tensor stays inside test_fp32_gpu.py's per-tensor floor of the Winograd path
    (PT_FLOOR, 1e-2), the median inside its STEP_MED_FLOOR (1e-2). The fused layers' folds change
    the rounding of their dy; the three-launch layers' do not (test_engine_three_launch_fold_bit_equal).
    Batch 8 leaves layer4 out (8 tiles: no Winograd weight gradient), batch 32 brings it in.
    With float-atomic BN sums two runs of ONE build already differ by the order of the atomics,
    amplified by the random-init network: the bar there is the one test_fp32_gpu.py sets for this
    undamped network, STEP_FLOOR (1.5e-2) on the worst tensor. Measured: deterministic median
    1.4e-5 / 4.1e-5, worst 9.2e-5 / 1.8e-4 (batch 8 / 32); atomic batch 8 median 4.2e-3, worst 5.8e-3."""
    from .test_fp32_gpu import PT_FLOOR, STEP_FLOOR, STEP_MED_FLOOR
    e1, layout, o1 = _step(monkeypatch, "", B, deterministic)
    e0, _, o0 = _step(monkeypatch, "wino_bwdfold=0", B, deterministic)
    assert sorted(e1.plan.dz_names()) == sorted(e0.plan.dz_names()) == THREE_LAUNCH[B]
    folded = [n for n in THREE_LAUNCH[B] if n in e1.plan.bwd_fold_names()]
    assert folded and not any(n.endswith(".0.conv2") for n in folded), folded  # behind a BN pair: no fold
    assert not e0.plan.bwd_fold_names()
    if deterministic:
        assert o1[0][0] == o0[0][0]
    errs = _per_tensor(layout, o1[0][1], o0[0][1])
    print("B=%d folded %s: median %.2e, worst %s" % (B, folded, errs[len(errs) // 2][0], errs[-3:]))
    assert errs[-1][0] <= (PT_FLOOR["1"] if deterministic else STEP_FLOOR), errs[-3:]
    assert errs[len(errs) // 2][0] <= STEP_MED_FLOOR, errs


def test_engine_side_stream_keeps_old_launches(monkeypatch):
    """With the weight gradients on the side stream (PSX_TUNE=wgrad_stream=1) no layer takes the
    merged transform or its fold: the three-launch sequence of before, whose result the merged
    plain transform on the compute stream reproduces bit for bit (deterministic mode)."""
    B = 8
    es, _, os_ = _step(monkeypatch, "wgrad_stream=1,wino_bwdfold=0", B)
    assert es.plan.wgrad_stream and es.wg_stream is not None and not es.plan.dz_names()
    ed, _, od = _step(monkeypatch, "wgrad_stream=1", B)
    assert not ed.plan.dz_names() and not any(n in ed.plan.bwd_fold_names() for n in THREE_LAUNCH[B]), \
        ed.plan.bwd_fold_names()
    em, _, om = _step(monkeypatch, "wgrad_stream=0,wino_bwdfold=0", B)
    assert not em.plan.wgrad_stream and em.wg_stream is None and sorted(em.plan.dz_names()) == THREE_LAUNCH[B]
    assert os_[0][0] == om[0][0]
    assert torch.equal(bits(os_[0][1]), bits(om[0][1]))
    # and with every fold on: the main-stream engine folds the three-launch layers, the side-stream
    # one writes their dy; the same bytes
    ef, _, of = _step(monkeypatch, "wgrad_stream=0", B)
    assert any(n in ef.plan.bwd_fold_names() for n in THREE_LAUNCH[B])
    assert torch.equal(bits(od[0][1]), bits(of[0][1]))


def test_engine_three_launch_fold_bit_equal(monkeypatch):
    """The three-launch layers' fold alone (EngineOptions bwd_fold="dz_only": the engine's other
    folds off): the step equals the unfolded one bit for bit, loss and gradient bytes
    (deterministic mode)."""
    B = 32
    _, _, o0 = _step(monkeypatch, "wino_bwdfold=0", B)
    e1, _, o1 = _step(monkeypatch, "", B, bwd_fold="dz_only")
    assert sorted(e1.plan.bwd_fold_names()) == ["layer3.1.conv1", "layer3.1.conv2", "layer4.1.conv1"], \
        e1.plan.bwd_fold_names()
    assert o1[0][0] == o0[0][0]
    assert torch.equal(bits(o1[0][1]), bits(o0[0][1]))


def test_engine_deterministic_steps_repeat(monkeypatch):
    """Two identical steps (a fresh engine each: an engine carries the BN statistics' shift from
    step to step) in deterministic mode: the same loss and gradient bytes."""
    e, _, a = _step(monkeypatch, "", 8, deterministic=True)
    assert e.plan.dz_names() and any(n in e.plan.bwd_fold_names() for n in e.plan.dz_names())
    _, _, b = _step(monkeypatch, "", 8, deterministic=True)
    assert a[0][0] == b[0][0]
    assert torch.equal(bits(a[0][1]), bits(b[0][1]))
