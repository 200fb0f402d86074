"""The per-launch specialisations of the fused fp32 Winograd conv (csrc/kernels/wino_fused.hip: the
input kind PLAIN / BNIN / BWDIN and the V side output HASV are template parameters, the group loop
has no dummy group): every instantiation psx_wino_fused's dispatch tables can reach, at the smallest
shapes that reach the code (one 16-tile workgroup per channel block), against torch float64 at the
bar of test_wino_fused_gpu.py; every activation-sized operand (x, res, y1, o, y2, ybn), the slot
sums and every output sit in front of a NaN guard region that must survive the launch (the weights
and the per-channel vectors do not: all of them but the flat residual load go through bounded
buffer descriptors anyway), and every output starts as NaN and must end finite."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from psx.ops import kernels as K  # noqa: E402

from .test_wino_fused_gpu import DEV, TOL, _bn_in, _bwd_case, _bwd_ref, _rel, _uf  # noqa: E402

GUARD = 4096
# (N, H = W, C = K): T = 16 tiles with border and interior tiles; every tile a border tile; two
# channel blocks and 8 groups
S_ONE, S_BORDER, S_WIDE = (1, 16, 64), (4, 8, 64), (1, 16, 128)


class Guarded:
    """Tensors allocated in front of a NaN guard region."""

    def __init__(self):
        self.guards = []

    def __call__(self, t):
        buf = torch.cat([t.reshape(-1).float(), torch.full((GUARD,), float("nan"), device=DEV)])
        self.guards.append(buf[t.numel():])
        return buf[:t.numel()].view(t.shape)

    def nan(self, *shape):
        return self(torch.full(shape, float("nan"), device=DEV))

    def intact(self):
        return all(bool(torch.isnan(g).all()) for g in self.guards)


def _operand(kind, nb, h, c, seed, G):
    """(the launch's x, its keyword arguments, the conv operand in float64 [nb][h][h][c], extras)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "plain":
        x = G(torch.relu(torch.randn(nb, h, h, c, device=DEV, generator=g)))
        return x, {}, x.double(), None
    if kind == "bnin":  # the previous layer's training BN + ReLU from its shifted slot sums
        z = G(torch.randn(nb, h, h, c, device=DEV, generator=g) * 2 + 0.5)
        t = _bn_in(c, seed=seed)
        zs = z - t["ssh"]
        sl = torch.zeros(K.STAT_SLOTS, 2, c, device=DEV)
        sl[0, 0] = zs.sum((0, 1, 2))
        sl[1, 1] = (zs * zs).sum((0, 1, 2)) / 2
        sl[2, 1] = (zs * zs).sum((0, 1, 2)) / 2
        fin = K.bn_fin(t["gamma"], t["beta"], t["rm"], t["rv"], t["affine"], t["saved"], t["ctr"].data_ptr(),
                       nb * h * h, 1e-5, 0.1, c, sshift=t["ssh"], sshift_next=t["ssh_next"])
        mean, var = z.double().mean((0, 1, 2)), z.double().var((0, 1, 2), unbiased=False)
        op = torch.relu((z.double() - mean) / torch.sqrt(var + 1e-5) * t["gamma"].double() + t["beta"].double())
        return z, {"bn_in": (G(sl), fin)}, op, t
    dz, yb, saved, gamma, part = _bwd_case(nb, h, c, seed=seed)  # bwdin
    t = {"coef": torch.full((3, c), float("nan"), device=DEV), "dgb": torch.full((2, c), float("nan"), device=DEV),
         "ctr": torch.zeros(4, dtype=torch.int32, device=DEV), "gamma": gamma, "saved": saved}
    fin = K.bn_bwd_fin(gamma, saved, t["coef"], t["dgb"][0].data_ptr(), t["dgb"][1].data_ptr(), t["ctr"].data_ptr(),
                       nb * h * h, 1.0, c, False)
    op, sxh, sdz = _bwd_ref(dz, yb, saved, gamma, part, nb * h * h)
    t["sxh"], t["sdz"] = sxh, sdz
    return G(dz), {"bwd_in": (G(yb), G(part), fin)}, op, t


def _conv_ref(op, w, bwd):
    """float64 NHWC result: the forward conv, or the data gradient (w [k][c] applied to a k-channel operand)."""
    if bwd:
        nb, h = op.shape[0], op.shape[1]
        g = torch.nn.grad.conv2d_input((nb, w.shape[1], h, h), w.double(), op.permute(0, 3, 1, 2), padding=1)
        return g.permute(0, 2, 3, 1)
    return F.conv2d(op.permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)


def _check_fwd(shape, res, kind, vout, seed):
    nb, h, c = shape
    torch.manual_seed(seed)
    G = Guarded()
    x, kw, op, keep = _operand(kind, nb, h, c, seed, G)  # keep: the tensors the BnFin points to
    w = torch.randn(c, c, 3, 3, device=DEV) * (2.0 / (9 * c)) ** 0.5
    uf, _u0 = _uf(w, c, c)
    r = G(torch.randn(nb, h, h, c, device=DEV)) if res else None
    ref = _conv_ref(op, w, False) + (r.double() if res else 0)
    y = G.nan(nb, h, h, c)
    stats = G(torch.zeros(K.STAT_SLOTS, 2, c, device=DEV))
    v = G.nan(K.wino_v_floats(nb, h, h, c)) if vout else None
    K.wino_fused(x, uf, y, r, stats, v, nb, h, h, c, c, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.isfinite(stats).all() and (v is None or torch.isfinite(v).all())
    assert G.intact()
    assert _rel(y, ref) < TOL
    s = stats.double().sum(0)
    assert torch.allclose(s[0], ref.sum((0, 1, 2)), rtol=1e-4, atol=1e-3 * ref.abs().max().item())
    assert torch.allclose(s[1], (ref ** 2).sum((0, 1, 2)), rtol=1e-4)
    return x, uf, y, r, stats, v, kw, w, keep


@pytest.mark.parametrize("vout", [False, True])
@pytest.mark.parametrize("kind", ["plain", "bnin"])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [S_ONE, S_WIDE])
def test_every_forward_instantiation(shape, res, kind, vout):
    _check_fwd(shape, res, kind, vout, seed=11 + shape[2] + 2 * res + vout)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [S_ONE, S_WIDE])
def test_forward_epilogue_with_bwd_fold(shape, res):
    """BWDIN with the forward epilogue (no consumer BN sums), as the first block's data gradient runs."""
    _check_fwd(shape, res, "bwdin", False, seed=5 + shape[2] + res)


@pytest.mark.parametrize("kind", ["plain", "bnin"])
def test_all_border_tiles(kind):
    _check_fwd(S_BORDER, False, kind, True, seed=3)


def _check_bwd(shape, res, maff, two, kind, seed, det=False):
    nb, h, c = shape
    torch.manual_seed(seed)
    G = Guarded()
    x, kw, op, t = _operand(kind, nb, h, c, seed, G)
    w = torch.randn(c, c, 3, 3, device=DEV) * (2.0 / (9 * c)) ** 0.5
    uf, _u0 = _uf(w, c, c, flip=True)
    r = G(torch.randn(nb, h, h, c, device=DEV)) if res else None
    o, y1, y2 = (G(torch.randn(nb, h, h, c, device=DEV)) for _ in range(3))
    saved1 = torch.stack([torch.randn(c, device=DEV), torch.rand(c, device=DEV) + 0.5])
    saved2 = torch.stack([torch.randn(c, device=DEV), torch.rand(c, device=DEV) + 0.5])
    aff = torch.stack([torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)]).contiguous()
    nst = 3 if two else 2
    part = G(torch.zeros(K.STAT_SLOTS * (K.det_slot_scale() if det else 1), nst, c, device=DEV))
    bst = K.bwd_stats_desc(part, None if maff else o, y1, saved1, y2 if two else None, saved2 if two else None,
                           mask_store=True, mask_aff=aff if maff else None)
    dx = G.nan(nb, h, h, c)
    K.wino_fused(x, uf, dx, r, None, None, nb, h, h, c, c, bst=bst, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    assert G.intact()
    g = _conv_ref(op, w, True) + (r.double() if res else 0)
    pos = (y1.double() * aff[0].double() + aff[1].double() > 0) if maff else (o.double() > 0)
    dz = torch.where(pos, g, torch.zeros_like(g))
    assert _rel(dx, dz) < TOL
    s = (K.det_slot_values(part, (K.STAT_SLOTS, nst, c)) if det else part.double()).sum(0)
    sums = [dz.sum((0, 1, 2)), (dz * (y1.double() - saved1[0].double()) * saved1[1].double()).sum((0, 1, 2))]
    if two:
        sums.append((dz * (y2.double() - saved2[0].double()) * saved2[1].double()).sum((0, 1, 2)))
    for i, ref in enumerate(sums):
        assert _rel(s[i], ref) < 1e-4, i
    if kind == "bwdin":  # the launch publishes the folded BN's dgamma / dbeta
        assert torch.allclose(t["dgb"][0].double(), t["sxh"], rtol=1e-5, atol=1e-5)
        assert torch.allclose(t["dgb"][1].double(), t["sdz"], rtol=1e-5, atol=1e-5)
    return dx, part


@pytest.mark.parametrize("kind", ["plain", "bwdin"])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("maff", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [S_ONE, S_WIDE])
def test_every_data_gradient_instantiation(shape, res, maff, two, kind):
    _check_bwd(shape, res, maff, two, kind, seed=7 + shape[2] + 8 * res + 4 * maff + 2 * two)


def test_data_gradient_all_border_tiles():
    _check_bwd(S_BORDER, True, False, False, "bwdin", seed=2)


def test_traits_of_the_other_direction_are_refused():
    """V and BNIN belong to the forward, V never goes with BWDIN: psx_wino_fused returns -3 (the
    binding raises HipError), it does not run another kernel. The outputs stay untouched."""
    from psx.ops._lib import HipError

    nb, h, c = S_ONE
    G = Guarded()
    x = torch.randn(nb, h, h, c, device=DEV)
    w = torch.randn(c, c, 3, 3, device=DEV)
    uf, _ = _uf(w, c, c)
    part = torch.zeros(K.STAT_SLOTS, 2, c, device=DEV)
    bst = K.bwd_stats_desc(part, x, x, torch.ones(2, c, device=DEV), mask_store=True)
    _, bn_kw, _, keep_bn = _operand("bnin", nb, h, c, 1, G)
    _, bwd_kw, _, keep_bwd = _operand("bwdin", nb, h, c, 1, G)
    refused = [dict(v=True, bst=bst),            # V with a data gradient
               dict(v=False, bst=bst, **bn_kw),   # BNIN with a data gradient
               dict(v=True, **bwd_kw)]            # V with BWDIN
    for kw in refused:
        y = torch.full_like(x, float("nan"))
        v = torch.full((K.wino_v_floats(nb, h, h, c),), float("nan"), device=DEV) if kw.pop("v") else None
        with pytest.raises(HipError, match="code -3"):
            K.wino_fused(x, uf, y, None, None, v, nb, h, h, c, c, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and (v is None or torch.isnan(v).all())


@pytest.mark.parametrize("kind", ["plain", "bnin"])
@pytest.mark.parametrize("shape", [S_ONE, S_BORDER, S_WIDE])
def test_v_output_changes_nothing_else(shape, kind):
    """HASV on and off on the same inputs: y and the BN slot sums bit-equal; V is the three-launch
    path's transformed input of the same inputs (BNIN: the same slot sums and BnFin folded into
    wino_conv's input transform), at the bar of test_wino_fused_gpu.py."""
    nb, h, c = shape
    x, uf, y1, _, st1, v, kw, w, _keep = _check_fwd(shape, False, kind, True, seed=21)
    y0 = torch.full_like(y1, float("nan"))
    st0 = torch.zeros(K.STAT_SLOTS, 2, c, device=DEV)
    K.wino_fused(x, uf, y0, None, st0, None, nb, h, h, c, c, **kw)
    torch.cuda.synchronize()
    # float-atomic slot sums: one workgroup per (slot, channel) at these shapes, so the order is fixed
    assert torch.equal(y0, y1) and torch.equal(st0, st1)
    _, u0 = _uf(w, c, c)
    v0 = torch.full_like(v, float("nan"))
    p0 = torch.empty(K.wino_p_floats(nb, h, h, c, c), device=DEV)
    K.wino_conv(x, u0, torch.empty_like(y1), None, None, v0, p0, nb, h, h, c, c, **kw)
    torch.cuda.synchronize()
    err = _rel(v, v0)
    print(f"V fused vs three-launch ({kind}, {shape}): {err:.3g}")
    assert err < 1e-6


@pytest.mark.parametrize("shape", [S_ONE, S_BORDER, S_WIDE])
def test_plain_equals_identity_bn(shape):
    """PLAIN uses the patch as loaded; BNIN with scale 1 and a shift that keeps every value positive
    (the ReLU never clips) must give the same conv, zero padding included: both against float64."""
    nb, h, c = shape
    torch.manual_seed(31)
    shift = 8.0
    z = torch.randn(nb, h, h, c, device=DEV).clamp_(-4, 4)
    w = torch.randn(c, c, 3, 3, device=DEV) * (2.0 / (9 * c)) ** 0.5
    uf, _ = _uf(w, c, c)
    mean, var = z.double().mean((0, 1, 2)), z.double().var((0, 1, 2), unbiased=False)
    t = _bn_in(c, seed=4)
    t["gamma"].copy_(torch.sqrt(var + 1e-5))  # scale = gamma * invstd = 1
    t["beta"].copy_(mean + shift)             # shift = beta - mean * scale = 8
    zs = z - t["ssh"]
    sl = torch.zeros(K.STAT_SLOTS, 2, c, device=DEV)
    sl[0, 0], sl[1, 1] = zs.sum((0, 1, 2)), (zs * zs).sum((0, 1, 2))
    fin = K.bn_fin(t["gamma"], t["beta"], t["rm"], t["rv"], t["affine"], t["saved"], t["ctr"].data_ptr(), nb * h * h,
                   1e-5, 0.1, c, sshift=t["ssh"], sshift_next=t["ssh_next"])
    opb = (z.double() - mean) / torch.sqrt(var + 1e-5) * t["gamma"].double() + t["beta"].double()
    assert opb.min().item() > 1.0
    yb = torch.full((nb, h, h, c), float("nan"), device=DEV)
    K.wino_fused(z, uf, yb, None, None, None, nb, h, h, c, c, bn_in=(sl, fin))
    xp = (z + shift).contiguous()
    yp = torch.full((nb, h, h, c), float("nan"), device=DEV)
    K.wino_fused(xp, uf, yp, None, None, None, nb, h, h, c, c)
    torch.cuda.synchronize()
    assert _rel(yb, _conv_ref(opb, w, False)) < TOL
    assert _rel(yp, _conv_ref(xp.double(), w, False)) < TOL
    assert _rel(yb, yp) < 2 * TOL + 1e-6  # each within TOL of float64 convs whose operands differ by fp32 rounding


def test_deterministic_launches_repeat():
    """Deterministic mode: two launches bit-equal, y and slot sums, for one forward and one
    two-BN data gradient."""
    nb, h, c = S_ONE
    try:
        K.set_deterministic(True)
        out = []
        for _ in range(2):
            y, stats = _check_fwd_det(nb, h, c)
            dx, part = _check_bwd(S_ONE, True, False, True, "plain", seed=9, det=True)
            out.append((y.clone(), stats.clone(), dx.clone(), part.clone()))
    finally:
        K.set_deterministic(None)
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_fwd_det(nb, h, c):
    torch.manual_seed(13)
    x = torch.relu(torch.randn(nb, h, h, c, device=DEV))
    w = torch.randn(c, c, 3, 3, device=DEV) * (2.0 / (9 * c)) ** 0.5
    uf, _ = _uf(w, c, c)
    y = torch.full((nb, h, h, c), float("nan"), device=DEV)
    stats = torch.zeros(K.STAT_SLOTS * K.det_slot_scale(), 2, c, device=DEV)
    K.wino_fused(x, uf, y, None, stats, None, nb, h, h, c, c)
    torch.cuda.synchronize()
    ref = _conv_ref(x.double(), w, False)
    assert _rel(y, ref) < TOL
    fixed = K.det_slot_values(stats, (K.STAT_SLOTS, 2, c)).sum(0)
    assert torch.allclose(fixed[0], ref.sum((0, 1, 2)), rtol=1e-4, atol=1e-3 * ref.abs().max().item())
    return y, stats
