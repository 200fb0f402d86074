"""The fp64 references of the conv v2 kernels (csrc/kernels/conv_v2.hip), the operands that make a
comparison with them exact, the case tables of tests/test_conv_paths_gpu.py, and the CPU tests
that give all of it its meaning. Everything public here is shared with the GPU module.

Exact operands. With small integer operands every product and every partial sum of a conv is an
integer below 2^24, exact in fp32 in any summation order (on the MFMA as well), so an fp32 kernel
must reproduce the float64 reference bit for bit and a bf16 kernel must equal
``ref.float().to(torch.bfloat16)`` (round to nearest even, common.hpp f2bf). The same holds for the
BN statistic slots (integer shifts) and the BN-backward slots (integer means, power-of-two invstd).
build_case asserts the conditions; a case that breaks one is a wrong case.

Operands are built on the host (build_wf, build_wd: the layouts optim.hip's unpack kernels document),
never through K.param_unpack, so a packing bug and a gather bug cannot cancel.

Slot rows. A partial sum lands in slot row (workgroup's pixel tile index) & 7: the in-kernel
epilogue's tile of BN pixels, the split-K epilogue's 32 pixels per workgroup, and for the parity
classes (MODE 3) the class-local tile index (slot_rows).

Numerics cases (random bf16-representable operands) hold an element to
    (n + 1) 2u (sum |w||x| + |res|)  [+ half a bf16 ulp of the reference]
with n the real products plus the adds of the splits and the residual; the factor 2 over the
any-order bound allows accumulate steps that truncate (stated, not tuned)."""
from dataclasses import dataclass, replace
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

from .test_bn_cpu import BF16, F32, SLOTS, U
from .test_sgd_cpu import within

LIM = 2.0 ** 24


# ---------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    """One launch. h, w: the forward conv's input image (= dx for a data gradient); ic, oc: the
    forward conv's channels. expect: (key, value) pairs K.conv2_path must report under ``tune``."""
    id: str
    dir: str            # "fwd", "dgrad", "dgrad_sc"
    f32: bool
    n: int
    h: int
    w: int
    ic: int
    oc: int
    k: int = 3
    stride: int = 1
    pad: int = 1
    tune: str = ""
    expect: tuple = ()
    res: bool = False
    stats: bool = False     # fwd: BN statistic slots
    sshift: bool = False
    fin: bool = False       # fwd: fuse_fin
    bst: int = 0            # dgrad: BN-backward sums, 2 or 3 of them
    mask: bool = False      # mask_store
    det: bool = False       # deterministic mode
    seed: int = 0
    xlim: int = 3           # exact operands: activations in [-xlim, xlim], weights in [-wlim, wlim]
    wlim: int = 2

    @property
    def dtype(self):
        return F32 if self.f32 else BF16

    @property
    def ks(self):
        return 32 if self.f32 else 64

    @property
    def epc(self):
        return 4 if self.f32 else 8

    @property
    def ohw(self):
        return ((self.h + 2 * self.pad - self.k) // self.stride + 1,
                (self.w + 2 * self.pad - self.k) // self.stride + 1)

    @property
    def kg(self):
        """Row length of the launch's weight operand (wf forward, wd backward), zero padded."""
        c = self.ic if self.dir == "fwd" else self.oc
        return -(-(self.k * self.k * c) // self.ks) * self.ks

    @property
    def out_shape(self):
        oh, ow = self.ohw
        return (self.n, oh, ow, self.oc) if self.dir == "fwd" else (self.n, self.h, self.w, self.ic)

    def path_args(self):
        return (self.dir, self.n, self.h, self.w, self.ic, self.oc, self.k, self.stride, self.pad, self.kg, self.f32)


def query_path(case, monkeypatch):
    """K.conv2_path of the case under its PSX_TUNE (read with getenv at every call), checked
    against what the case names. Host code only: runs without a GPU."""
    from psx.ops import kernels as K
    if case.tune:
        monkeypatch.setenv("PSX_TUNE", case.tune)
    else:
        monkeypatch.delenv("PSX_TUNE", raising=False)
    path = K.conv2_path(*case.path_args())
    assert isinstance(path, dict), (case.id, "refused", path)
    for key, val in case.expect:
        assert path[key] == val, (case.id, key, "planner took", path)
    return path


# ---------------------------------------------------------------------------- host-built operands
def build_wf(w, ks):
    """OIHW -> the forward operand [OC][Kg]: wf[oc][tap * Cp + c], tap = r * S + s, Kg the row
    length R S Cp rounded up to whole k-steps of ks elements with zeros (optim.hip unpack_chunk)."""
    oc, cp, R, S = w.shape
    kg = -(-(R * S * cp) // ks) * ks
    out = torch.zeros(oc, kg, dtype=w.dtype)
    out[:, :R * S * cp] = w.permute(0, 2, 3, 1).reshape(oc, R * S * cp)
    return out


def build_wd(w, ks):
    """OIHW -> the data-gradient operand [Cp][Kgd]: wd[c][tap * OC + oc] (zero padded to whole
    k-steps: the engine's layers have R S OC % 64 == 0, the small-OC test layers do not)."""
    oc, cp, R, S = w.shape
    kgd = -(-(R * S * oc) // ks) * ks
    out = torch.zeros(cp, kgd, dtype=w.dtype)
    out[:, :R * S * oc] = w.permute(1, 2, 3, 0).reshape(cp, R * S * oc)
    return out


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------- fp64 references
def fwd_reference(x, w, stride, pad):
    """x NCHW, w OIHW (any dtype, decoded exactly) -> float64 NHWC [N][OH][OW][OC]."""
    return nhwc(F.conv2d(x.double(), w.double(), stride=stride, padding=pad))


def dgrad_reference(dy, w, hw, stride, pad, res=None, dy_sc=None, w_sc=None):
    """Data gradient, float64 NHWC [N][H][W][IC]: dy NCHW [N][OC][P][Q] against w OIHW, any stride
    1 or 2, any pad, non-square; + res (NHWC); + the folded 1x1 / stride-2 / pad-0 shortcut's data
    gradient of dy_sc against w_sc."""
    n, ic = dy.shape[0], w.shape[1]
    dx = torch.nn.grad.conv2d_input((n, ic) + tuple(hw), w.double(), dy.double(), stride=stride, padding=pad)
    if dy_sc is not None:
        dx = dx + torch.nn.grad.conv2d_input((n, ic) + tuple(hw), w_sc.double(), dy_sc.double(), stride=2, padding=0)
    dx = nhwc(dx)
    return dx + res.double() if res is not None else dx


def naive_fwd(x, w, stride, pad):
    n, ic, H, W = x.shape
    oc, _, R, S = w.shape
    oh, ow = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    y = torch.zeros(n, oh, ow, oc, dtype=torch.float64)
    for b in range(n):
        for i in range(oh):
            for j in range(ow):
                for o in range(oc):
                    for c in range(ic):
                        for r in range(R):
                            for s in range(S):
                                ih, iw = i * stride - pad + r, j * stride - pad + s
                                if 0 <= ih < H and 0 <= iw < W:
                                    y[b, i, j, o] += float(x[b, c, ih, iw]) * float(w[o, c, r, s])
    return y


def naive_dgrad(dy, w, hw, stride, pad):
    n, oc, P, Q = dy.shape
    ic, R, S = w.shape[1], w.shape[2], w.shape[3]
    dx = torch.zeros(n, hw[0], hw[1], ic, dtype=torch.float64)
    for b in range(n):
        for i in range(P):
            for j in range(Q):
                for o in range(oc):
                    for c in range(ic):
                        for r in range(R):
                            for s in range(S):
                                ih, iw = i * stride - pad + r, j * stride - pad + s
                                if 0 <= ih < hw[0] and 0 <= iw < hw[1]:
                                    dx[b, ih, iw, c] += float(dy[b, o, i, j]) * float(w[o, c, r, s])
    return dx


# ---------------------------------------------------------------------------- slot rows
def slot_rows(path, n, H, W):
    """Slot row of every output pixel [n H W] (flat NHW order) under the launch ``path``."""
    pix = torch.arange(n * H * W)
    if path["splits"] > 1:      # conv_splitk_epilogue: blockIdx.x & 7, 32 pixels per workgroup
        return (pix // 32) % SLOTS
    if path["mode"] != 3:       # in-kernel epilogue: pixel tile index & 7
        return (pix // path["bn"]) % SLOTS
    rows = torch.zeros(n, H, W, dtype=torch.long)
    for py in range(2):         # parity classes: the class-local tile index
        for px in range(2):
            CH, CW = (H - py + 1) // 2, (W - px + 1) // 2
            if CH * CW == 0:
                continue
            loc = torch.arange(n * CH * CW).view(n, CH, CW)
            rows[:, py::2, px::2] = (loc // path["bn"]) % SLOTS
    return rows.reshape(-1)


def workgroup_of(path, n, H, W):
    """(workgroup id of every output pixel, number of ids): the unit whose per-channel partial
    total is one add into a slot row (deterministic mode: one fixed-point add). id % 8 is NOT the
    slot row for the parity classes; use slot_rows for that."""
    pix = torch.arange(n * H * W)
    if path["splits"] > 1:
        return pix // 32, -(-n * H * W // 32)
    if path["mode"] != 3:
        return pix // path["bn"], -(-n * H * W // path["bn"])
    wg = torch.zeros(n, H, W, dtype=torch.long)
    base = 0
    for py in range(2):
        for px in range(2):
            CH, CW = (H - py + 1) // 2, (W - px + 1) // 2
            if CH * CW == 0:
                continue
            loc = torch.arange(n * CH * CW).view(n, CH, CW) // path["bn"]
            wg[:, py::2, px::2] = base + loc
            base += int(loc.max()) + 1
    return wg.reshape(-1), base


def fwd_stats_reference(stored, rows, sshift=None):
    """Per slot row (sum (y - k), sum (y - k)^2) of the STORED values, float64 [8][2][C]."""
    C = stored.shape[-1]
    d = stored.double().reshape(-1, C)
    if sshift is not None:
        d = d - sshift.double()
    out = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    out[:, 0].index_add_(0, rows, d)
    out[:, 1].index_add_(0, rows, d * d)
    return out


def bwd_terms(g, o, y1, saved1, y2=None, saved2=None, ge=False):
    """dz = g [o > 0] and the terms dz, dz xhat1 [, dz xhat2] per pixel, float64 [NS][npix][C]."""
    C = g.shape[-1]
    od = o.double().reshape(-1, C)
    dz = g.double().reshape(-1, C) * ((od >= 0) if ge else (od > 0)).double()
    t = [dz, dz * (y1.double().reshape(-1, C) - saved1[0].double()) * saved1[1].double()]
    if y2 is not None:
        t.append(dz * (y2.double().reshape(-1, C) - saved2[0].double()) * saved2[1].double())
    return torch.stack(t)


def bwd_sums_reference(g, rows, o, y1, saved1, y2=None, saved2=None, ge=False):
    """Per slot row (sum dz, sum dz xhat1 [, sum dz xhat2]) of the STORED gradient g, [8][NS][C]."""
    t = bwd_terms(g, o, y1, saved1, y2, saved2, ge)
    out = torch.zeros(SLOTS, t.shape[0], g.shape[-1], dtype=torch.float64)
    for k in range(t.shape[0]):
        out[:, k].index_add_(0, rows, t[k])
    return out


# ---------------------------------------------------------------------------- operands of a case
def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).double()


def _bf(gen, shape, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(BF16).double()


def half_bf16_ulp(ref):
    _, e = torch.frexp(ref.abs().float())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e.to(torch.int32) - 9))


MARK_X = 5.0  # the marked activations: +-5 against an odd weight in [201, 255]


def _marks(n, gi, gj):
    """(b, i, j) of the marked grid points: the first, the middle and the last."""
    G = n * gi * gj
    flat = torch.tensor(sorted({0, G // 2, G - 1}))
    return flat // (gi * gj), (flat // gj) % gi, flat % gj


def mark_odd_outputs(c, gen, act, res):
    """Operands of a bf16 exact case with statistics, which must have in every channel an output
    that bf16 rounding changes (otherwise 'sums of the stored values' is not tested). Any odd
    integer above 256 is such a value. So: even weights and an even residual, except one tap,
    (pad, pad) of gathered channel 0, whose weight is odd in [201, 255] for every output channel;
    the gathered channel 0 of ``act`` (changed in place) is zero except +-5 at up to three marked
    pixels. The outputs under the marks are then odd, around 1000 to 1275 in magnitude, and
    everything else is even. Returns (w, res, (b, i, j) of the marked output pixels); build_case
    asserts the property."""
    assert 2 * c.pad < c.k
    oh, ow = c.ohw
    fwd = c.dir == "fwd"
    w = 2.0 * _ints(gen, (c.oc, c.ic, c.k, c.k), 1)
    if c.wlim < 2:  # a quarter of them nonzero
        w = w * (torch.rand(w.shape, generator=gen) < 0.25)
    if res is not None:
        res = 2.0 * _ints(gen, res.shape, 2)
    mb, mi, mj = _marks(c.n, oh, ow)
    sign = torch.where(torch.rand(mb.shape, generator=gen) < 0.5, -MARK_X, MARK_X).double()
    act[:, 0] = 0
    odd = 201.0 + 2 * torch.randint(0, 28, (c.oc if fwd else c.ic,), generator=gen).double()
    if fwd:   # out (b, i, j) reads x (b, i s, j s) through tap (pad, pad)
        act[mb, 0, mi * c.stride, mj * c.stride] = sign
        w[:, 0, c.pad, c.pad] = odd
        return w, res, (mb, mi, mj)
    act[mb, 0, mi, mj] = sign  # dy (b, i, j) reaches dx (b, i s, j s) through tap (pad, pad)
    w[0, :, c.pad, c.pad] = odd
    return w, res, (mb, mi * c.stride, mj * c.stride)


def build_case(case, path, numerics=False):
    """Operands, references and (numerics) bounds of one launch along ``path``. Exact cases draw
    x in [-xlim, xlim], w in [-wlim, wlim] (residual in [-4, 4]) and assert the exactness
    conditions; the bf16 cases with statistics are drawn by mark_odd_outputs, and with BN-backward
    sums the mask operand is positive under its marks."""
    c, gen = case, torch.Generator().manual_seed(case.seed + 1)
    oh, ow = c.ohw
    fwd = c.dir == "fwd"
    trick = not numerics and not c.f32 and (c.stats or bool(c.bst))
    act_shape = (c.n, c.ic, c.h, c.w) if fwd else (c.n, c.oc, oh, ow)
    draw = (lambda s, lim: _bf(gen, s)) if numerics else (lambda s, lim: _ints(gen, s, lim))
    act = draw(act_shape, c.xlim)
    wshape = (c.oc, c.ic, c.k, c.k)
    w = _bf(gen, wshape, (c.ic * c.k * c.k) ** -0.5) if numerics else _ints(gen, wshape, c.wlim)
    res = draw(c.out_shape, 4) if c.res else None
    marked = None
    if trick:
        w, res, marked = mark_odd_outputs(c, gen, act, res)
    d = dict(case=c, path=path, act=act, w=w)
    ones = torch.ones(1, 1, c.k, c.k, dtype=torch.float64)
    if fwd:
        ref = fwd_reference(act, w, c.stride, c.pad)
        mag = fwd_reference(act.abs(), w.abs(), c.stride, c.pad)
        nprod = fwd_reference(torch.ones(1, 1, c.h, c.w), ones, c.stride, c.pad) * c.ic
        d["wmat"] = build_wf(w, c.ks)
    else:
        sc = c.dir == "dgrad_sc"
        dy_sc = draw(act_shape, c.xlim) if sc else None
        w_sc = None
        if sc:
            w_sc = _bf(gen, (c.oc, c.ic, 1, 1), c.ic ** -0.5) if numerics else _ints(gen, (c.oc, c.ic, 1, 1), 1)
            w_sc = w_sc * (2.0 if trick else 1.0)  # even beside the marks
        ref = dgrad_reference(act, w, (c.h, c.w), c.stride, c.pad, res, dy_sc, w_sc)
        mag = dgrad_reference(act.abs(), w.abs(), (c.h, c.w), c.stride, c.pad, None if res is None else res.abs(),
                              None if dy_sc is None else dy_sc.abs(), None if w_sc is None else w_sc.abs())
        one_dy = torch.ones(1, 1, oh, ow, dtype=torch.float64)
        nprod = dgrad_reference(one_dy, ones, (c.h, c.w), c.stride, c.pad) * c.oc
        if sc:
            nprod = nprod + dgrad_reference(one_dy, ones[:, :, :1, :1], (c.h, c.w), 2, 0) * c.oc
            d.update(dy_sc=dy_sc, w_sc=w_sc, wmat_sc=build_wd(w_sc, c.ks))
        d["wmat"] = build_wd(w, c.ks)
    d.update(res=res, ref=ref, mag=mag)
    if numerics:
        nadd = nprod + (path["splits"] - 1) + (1 if c.res else 0)
        d["bound"] = (nadd + 1) * 2 * U * mag + (0 if c.f32 else half_bf16_ulp(ref))
        stored = ref.float().to(c.dtype)
    else:
        assert float(mag.max()) < LIM, (c.id, "sum |w||x| per output", float(mag.max()))
        stored = ref.float().to(c.dtype)
        if c.f32:
            assert torch.equal(stored.double(), ref)
    d["stored"] = stored
    C = c.out_shape[-1]
    rows = slot_rows(path, *c.out_shape[:3])
    d["rows"] = rows
    chg = (stored.double() != ref).reshape(-1, C)
    if c.stats:
        k = _ints(gen, (C,), 2).float() if c.sshift else None
        d["sshift"] = k
        if not numerics:
            dd = stored.double().reshape(-1, C) - (k.double() if k is not None else 0.0)
            assert float(dd.abs().sum(0).max()) < LIM and float((dd * dd).sum(0).max()) < LIM, \
                (c.id, "sum |d|, sum d^2 per channel", float(dd.abs().sum(0).max()), float((dd * dd).sum(0).max()))
        d["stats_ref"] = fwd_stats_reference(stored, rows, k)
        d["rounded"] = chg.any(0)
    if c.bst:
        shp = c.out_shape
        o = _ints(gen, shp, 2)                      # zeros among them: [o > 0] against [o >= 0]
        if marked is not None:
            o[marked[0], marked[1], marked[2]] = 1.0
        o = o.to(c.dtype)
        y1 = (_bf(gen, shp) if numerics else _ints(gen, shp, 4)).to(c.dtype)
        sv1 = torch.stack([_ints(gen, (C,), 2), 2.0 ** torch.randint(-1, 2, (C,), generator=gen).double()]).float()
        y2 = sv2 = None
        if c.bst == 3:
            y2 = (_bf(gen, shp) if numerics else _ints(gen, shp, 4)).to(c.dtype)
            sv2 = torch.stack([_ints(gen, (C,), 2), 2.0 ** torch.randint(-1, 2, (C,), generator=gen).double()]).float()
        d.update(o=o, y1=y1, y2=y2, saved1=sv1, saved2=sv2)
        t = bwd_terms(stored, o, y1, sv1, y2, sv2)
        if not numerics:  # terms are multiples of 1/2: exact below 2^23
            worst = float(t.abs().sum(1).max())
            assert worst < LIM / 2, (c.id, "sum |dz xhat| per channel", worst)
        d["bsums_ref"] = bwd_sums_reference(stored, rows, o, y1, sv1, y2, sv2)
        pos = (o.double() > 0).reshape(-1, C)
        d["rounded"] = (chg & pos).any(0)           # a rounded gradient that the mask lets through
        if c.mask:
            d["stored"] = torch.where(o.double() > 0, stored, torch.zeros_like(stored))  # +0 where masked
    if trick:
        assert bool(d["rounded"].all()), (c.id, "channels without a rounded output", int((~d["rounded"]).sum()))
    return d


@lru_cache(maxsize=None)
def _cached(case, path_items, numerics):
    return build_case(case, dict(path_items), numerics)


def case_data(case, path, numerics=False):
    """build_case, computed once per (case, path) and shared: callers leave it unchanged."""
    return _cached(case, tuple(sorted(path.items())), numerics)


# ---------------------------------------------------------------------------- case tables
def _c(id, dir, f32, n, h, w, ic, oc, **kw):
    return Case(id=id, dir=dir, f32=f32, n=n, h=h, w=w, ic=ic, oc=oc, **kw)


GEN0 = (("kind", "generic"), ("mode", 0), ("splits", 1))
GEN1 = (("kind", "generic"), ("mode", 1), ("splits", 1))
TILES = ((128, 128, 2), (128, 256, 2), (64, 128, 2), (64, 64, 2), (64, 256, 1), (64, 128, 1))


def _t(f32):
    return "f32" if f32 else "bf16"


def generic_cases():
    out = []
    for f32 in (False, True):
        e, t = (4 if f32 else 8), _t(f32)
        # non-uniform-tap gather (log2_icc < 3): IC e, 2e, 4e -> OC 64, at N 2, H 5, W 7
        for ic in (e, 2 * e, 4 * e):
            for s in (1, 2):
                # 2, 3 and 5 k-steps (bf16: Kg 72 / 144 / 288 -> 128 / 192 / 320)
                kps = -(-9 * ic // (32 if f32 else 64))
                out.append(_c(f"gather-ic{ic}-s{s}-{t}", "fwd", f32, 2, 5, 7, ic, 64, stride=s,
                              expect=GEN0 + (("kps", kps),),
                              stats=True))
        # the stem shape: Kg 49 e -> whole k-steps (zero-padded k columns, tap >= R*S)
        out.append(_c(f"stem7-{t}", "fwd", f32, 1, 19, 17, e, 64, k=7, stride=2, pad=3, expect=GEN0, stats=True,
                      sshift=True))
        ks = 32 if f32 else 64
        # uniform tap
        out.append(_c(f"utap-s2p1-{t}", "fwd", f32, 2, 9, 7, ks, 64, stride=2, expect=GEN0, stats=True))
        out.append(_c(f"utap-s2p0-{t}", "fwd", f32, 2, 7, 9, ks, 64, stride=2, pad=0, expect=GEN0, stats=True,
                      sshift=True))
        out.append(_c(f"utap-1x1s2-{t}", "fwd", f32, 2, 9, 7, ks, 64, k=1, stride=2, pad=0, expect=GEN0, stats=True))
        out.append(_c(f"gemm1x1-75-{t}", "fwd", f32, 3, 5, 5, ks, 64, k=1, pad=0, expect=GEN0, stats=True, fin=True))
        out.append(_c(f"gemm1x1-35-{t}", "fwd", f32, 1, 5, 7, ks, 64, k=1, pad=0, expect=GEN0 + (("pix_tiles", 1),),
                      stats=True))
        # ring depth: 1, 2, 4 k-steps (1x1) and 9 (3x3), statistics on; three k-steps, unsplit: the
        # gather cases above at IC 2e (Kg 144 -> 192 bf16, 72 -> 96 fp32), which pin kps = 3
        for nk in (1, 2, 4):
            out.append(_c(f"ring{nk}-{t}", "fwd", f32, 3, 5, 5, nk * ks, 64, k=1, pad=0, expect=GEN0 + (("kps", nk),),
                          stats=True, sshift=nk == 2))
        out.append(_c(f"ring9-{t}", "fwd", f32, 3, 5, 5, ks, 64, tune="cv_tapr=0", expect=GEN0 + (("kps", 9),),
                      stats=True))
        # dgrad on the generic mainloop (MODE 1), with and without residual
        for res in (False, True):
            r = "-res" if res else ""
            out.append(_c(f"dgrad-1x1{r}-{t}", "dgrad", f32, 3, 5, 5, 64, 2 * ks, k=1, pad=0, expect=GEN1, res=res))
            out.append(_c(f"dgrad-3x3{r}-{t}", "dgrad", f32, 2, 5, 7, 64, ks, tune="cv_tapr=0", expect=GEN1, res=res,
                          bst=2 if res else 0))
            out.append(_c(f"dgrad-gather{r}-{t}", "dgrad", f32, 2, 5, 7, 64, e, expect=GEN1, res=res))
        # every tile configuration of dispatch2, at 75 pixels and at three tiles with a partial last
        for bm, bn, wgm in TILES:
            if f32 and (bm, bn) == (128, 256):
                continue
            exp = (("bm", bm), ("bn", bn), ("wgm", wgm))
            tune = f"cv_bm={bm},cv_bn={bn},cv_wgm={wgm},cv_splits=1,cv_tapr=0"
            for tag, (n, h, w) in (("75", (3, 5, 5)), ("3t", (-(-(2 * bn + 1) // 35), 5, 7))):
                assert tag == "75" or (-(-n * h * w // bn) == 3 and (n * h * w) % bn)
                out.append(_c(f"tile{bm}x{bn}x{wgm}-{tag}-fwd-{t}", "fwd", f32, n, h, w, ks, 128, tune=tune,
                              expect=GEN0 + exp, stats=True))
                out.append(_c(f"tile{bm}x{bn}x{wgm}-{tag}-dgrad-{t}", "dgrad", f32, n, h, w, 128, ks, tune=tune,
                              expect=GEN1 + exp, res=True, bst=2))
    return out


def mode2_cases():
    out = []
    for f32 in (False, True):
        e, t = (4 if f32 else 8), _t(f32)
        exp = (("kind", "generic"), ("mode", 2), ("splits", 1))
        for oc in (e, 2 * e, 4 * e):
            for k, pad in ((3, 1), (1, 0)):
                for h, w in ((9, 7), (8, 8)):
                    out.append(_c(f"mode2-oc{oc}-k{k}-{h}x{w}-{t}", "dgrad", f32, 2, h, w, 64, oc, k=k, stride=2,
                                  pad=pad,
                                  expect=exp, res=(h == 9)))
    return out


def parity_cases():
    out = []
    P3 = (("kind", "generic"), ("mode", 3), ("splits", 1))
    for f32 in (False, True):
        t = _t(f32)
        for oc in (64, 128):
            for k, pad in ((3, 1), (1, 0)):
                for i, (n, h, w) in enumerate(((2, 8, 8), (2, 9, 7), (3, 7, 7), (5, 1, 1), (3, 2, 1))):
                    out.append(_c(f"parity-oc{oc}-k{k}-{h}x{w}-{t}", "dgrad", f32, n, h, w, 64, oc, k=k, stride=2,
                                  pad=pad, expect=P3, res=bool(i & 1), bst=(0, 2, 3)[i % 3], mask=(i == 2)))
        out.append(_c(f"parity-7x7-{t}", "dgrad", f32, 1, 9, 7, 64, 64, k=7, stride=2, pad=3, expect=P3))
        # class (0,0) one more tile than class (1,1): 9x15 at N 1 has 5x8 = 40 and 4x7 = 28 pixels... at N 2: 80 / 56
        out.append(_c(f"parity-tiles-{t}", "dgrad", f32, 2, 9, 15, 64, 64, stride=2, expect=P3 + (("bn", 64),
                                                                                                  ("pix_tiles", 2)),
                      res=True, bst=2))
        out.append(_c(f"parity-64x128-{t}", "dgrad", f32, 2, 9, 7, 64, 64, stride=2, tune="cv_bn=128",
                      expect=P3 + (("bm", 64), ("bn", 128)), bst=3))
        for i, (n, h, w) in enumerate(((2, 8, 8), (2, 9, 7), (3, 7, 7), (5, 1, 1), (3, 2, 1))):
            out.append(_c(f"fold-{h}x{w}-{t}", "dgrad_sc", f32, n, h, w, 64, 64, stride=2, expect=P3,
                          bst=(2, 0, 3)[i % 3], mask=(i == 2)))
    return out


def tapr_cases():
    out = []
    for f32 in (False, True):
        t = _t(f32)
        for W in (1, 2, 4, 8, 16, 32, 64):
            n = max(1, 128 // (W * W))                     # two 64-pixel tiles where an image is smaller
            if W == 4:
                n = 8                                      # four images per tile
            exp = (("kind", "tapr_rows"), ("bn", 64), ("splits", 1))
            ic = 64 if W >= 32 else (128 if W in (4, 8) else 64)
            wl = 1 if W >= 32 else 2                       # thousands of pixels: keep sum d^2 below 2^24
            out.append(_c(f"tapr-w{W}-fwd-{t}", "fwd", f32, n, W, W, ic, 64, expect=exp + (("mode", 0),), stats=True,
                          sshift=W == 4, fin=W == 8, wlim=wl))
            out.append(_c(f"tapr-w{W}-dgrad-{t}", "dgrad", f32, n, W, W, 64, ic, expect=exp + (("mode", 1),),
                          res=W != 2, bst=(2, 3)[W % 3 == 1] if W < 64 else 0, mask=W == 16, wlim=wl))
        for bn in (128, 256):
            exp = (("kind", "tapr_rows"), ("bn", bn), ("wgm", 1 if bn == 256 else 2))
            out.append(_c(f"tapr-bn{bn}-fwd-{t}", "fwd", f32, 2 * bn // 64, 8, 8, 64, 64, tune=f"cv_tapr_bn={bn}",
                          expect=exp + (("mode", 0),), stats=True))
            out.append(_c(f"tapr-bn{bn}-dgrad-{t}", "dgrad", f32, 2 * bn // 64, 8, 8, 64, 64, tune=f"cv_tapr_bn={bn}",
                          expect=exp + (("mode", 1),), res=True, bst=2))
    return out


# 3x7x7 = 147 pixels (partial last tile; the first tile's pix0 - 1 < 0), 35 (less than a tile),
# 196, one-pixel-wide and one-pixel-high images, 70 images of 1x1 and 128 pixels of 8x8 (both
# power-of-two squares, which take the halo mode only when it is forced)
HALO_SHAPES = ((3, 7, 7), (1, 5, 7), (1, 14, 14), (4, 1, 9), (4, 9, 1), (70, 1, 1), (2, 8, 8))


def halo_cases(off=False):
    """The halo shapes; ``off``: the same launches with cv_tapr_halo=0, which fall to the generic
    path and must agree with the halo result bit for bit."""
    out = []
    for f32 in (False, True):
        t = _t(f32)
        for i, (n, h, w) in enumerate(HALO_SHAPES):
            forced = h == w and not h & (h - 1)
            if off:
                tune, exp = ("cv_tapr=0" if forced else "cv_tapr_halo=0"), (("kind", "generic"),)
            else:
                tune, exp = ("cv_tapr_halo=1" if forced else ""), (("kind", "tapr_halo"), ("bn", 64), ("splits", 1))
            tag = "halo-off" if off else "halo"
            out.append(_c(f"{tag}-{n}x{h}x{w}-fwd-{t}", "fwd", f32, n, h, w, 64, 64, tune=tune,
                          expect=exp + (("mode", 0),),
                          stats=True, sshift=bool(i & 1), fin=(i == 0)))
            out.append(_c(f"{tag}-{n}x{h}x{w}-dgrad-{t}", "dgrad", f32, n, h, w, 64, 64, tune=tune,
                          expect=exp + (("mode", 1),), res=bool(i & 1), bst=(2, 3, 0)[i % 3], mask=(i == 3)))
    return out


def splitk_cases():
    out = []
    for f32 in (False, True):
        t, ks = _t(f32), (32 if f32 else 64)
        ic2 = 2 * ks                                            # 18 k-steps through a 3x3
        out.append(_c(f"splitk-natural-{t}", "fwd", f32, 2, 9, 7, ic2, 64, stride=2,
                      expect=(("kind", "generic"), ("mode", 0), ("splits", 2)), stats=True))
        for sp, kps in ((2, 5), (4, 3), (8, 2)):                # 9 k-steps: 5+4, 3+3+3+0, 2+2+2+2+1+0+0+0
            tune = f"cv_splits={sp},cv_tapr=0"
            exp = (("kind", "generic"), ("splits", sp), ("kps", kps))
            for npx, (n, h, w) in ((1, (1, 1, 1)), (33, (3, 11, 1)), (160, (5, 4, 8))):
                out.append(_c(f"splitk{sp}-{npx}-fwd-{t}", "fwd", f32, n, h, w, ks, 64, tune=tune,
                              expect=exp + (("mode", 0),),
                              stats=True, sshift=sp == 4, fin=sp == 2))
                out.append(_c(f"splitk{sp}-{npx}-dgrad-{t}", "dgrad", f32, n, h, w, 64, ks, tune=tune,
                              expect=exp + (("mode", 1),), res=sp != 4, bst=(2, 3)[sp == 8], mask=sp == 2))
        out.append(_c(f"splitk-oc2048-{t}", "fwd", f32, 3, 11, 1, ks, 2048, tune="cv_splits=2,cv_tapr=0",
                      expect=(("splits", 2),), stats=True))
    return out


def plain_cases():
    """Launches with neither statistics nor BN-backward sums: the epilogues' early exits
    (conv2_kernel's and conv_splitk_epilogue's `if (!st && !bwd) return`), forward on the generic,
    tap-reuse, halo and split-K paths and the split-K data gradient with and without residual."""
    out = []
    for f32 in (False, True):
        t, ks, e = _t(f32), (32 if f32 else 64), (4 if f32 else 8)
        SK = (("kind", "generic"), ("splits", 2), ("kps", 5))
        out += [
            _c(f"plain-gather-{t}", "fwd", f32, 2, 5, 7, 2 * e, 64, stride=2, expect=GEN0 + (("kps", 3),)),
            _c(f"plain-utap-{t}", "fwd", f32, 2, 9, 7, ks, 64, stride=2, expect=GEN0),
            _c(f"plain-gemm1x1-{t}", "fwd", f32, 3, 5, 5, ks, 64, k=1, pad=0, expect=GEN0),
            _c(f"plain-ring9-3t-{t}", "fwd", f32, 4, 5, 7, ks, 64, tune="cv_tapr=0", expect=GEN0 + (("pix_tiles", 3),)),
            _c(f"plain-tapr-w4-{t}", "fwd", f32, 8, 4, 4, 128, 64, expect=(("kind", "tapr_rows"), ("mode", 0), ("bn", 64))),
            _c(f"plain-tapr-bn128-{t}", "fwd", f32, 4, 8, 8, 64, 64, tune="cv_tapr_bn=128",
               expect=(("kind", "tapr_rows"), ("mode", 0), ("bn", 128))),
            _c(f"plain-halo-147-{t}", "fwd", f32, 3, 7, 7, 64, 64, expect=(("kind", "tapr_halo"), ("mode", 0))),
            _c(f"plain-halo-35-{t}", "fwd", f32, 1, 5, 7, 64, 64, expect=(("kind", "tapr_halo"), ("mode", 0))),
            _c(f"plain-splitk-natural-{t}", "fwd", f32, 2, 9, 7, 2 * ks, 64, stride=2,
               expect=(("kind", "generic"), ("mode", 0), ("splits", 2))),
        ]
        for npx, (n, h, w) in ((33, (3, 11, 1)), (160, (5, 4, 8))):
            out.append(_c(f"plain-splitk2-{npx}-fwd-{t}", "fwd", f32, n, h, w, ks, 64, tune="cv_splits=2,cv_tapr=0",
                          expect=SK + (("mode", 0),)))
            for res in (False, True):
                out.append(_c(f"plain-splitk2-{npx}-dgrad{'-res' if res else ''}-{t}", "dgrad", f32, n, h, w, 64, ks,
                              tune="cv_splits=2,cv_tapr=0", expect=SK + (("mode", 1),), res=res))
        out.append(_c(f"plain-splitk4-1-dgrad-{t}", "dgrad", f32, 1, 1, 1, 64, ks, tune="cv_splits=4,cv_tapr=0",
                      expect=(("kind", "generic"), ("mode", 1), ("splits", 4), ("kps", 3)), res=True))
    return out


def det_cases():
    out = []
    for f32 in (False, True):
        t, ks = _t(f32), (32 if f32 else 64)
        out += [
            _c(f"det-generic-fwd-{t}", "fwd", f32, 3, 5, 5, ks, 64, k=1, pad=0, expect=GEN0, stats=True, det=True,
               fin=True),
            _c(f"det-generic-dgrad-{t}", "dgrad", f32, 3, 5, 5, 64, ks, k=1, pad=0, expect=GEN1, bst=2, det=True),
            _c(f"det-tapr-fwd-{t}", "fwd", f32, 3, 8, 8, 64, 64, expect=(("kind", "tapr_rows"),), stats=True,
               sshift=True, det=True),
            _c(f"det-tapr-dgrad-{t}", "dgrad", f32, 3, 8, 8, 64, 64, expect=(("kind", "tapr_rows"),), bst=3, det=True),
            _c(f"det-halo-fwd-{t}", "fwd", f32, 3, 7, 7, 64, 64, expect=(("kind", "tapr_halo"),), stats=True, det=True),
            _c(f"det-halo-dgrad-{t}", "dgrad", f32, 3, 7, 7, 64, 64, expect=(("kind", "tapr_halo"),), bst=2,
               res=True, det=True),
            _c(f"det-parity-{t}", "dgrad", f32, 2, 9, 15, 64, 64, stride=2, expect=(("mode", 3),), bst=2, det=True),
            _c(f"det-splitk-fwd-{t}", "fwd", f32, 5, 4, 8, ks, 64, tune="cv_splits=2,cv_tapr=0", expect=(("splits",
                                                                                                          2),),
               stats=True, det=True, fin=True),
            _c(f"det-splitk-dgrad-{t}", "dgrad", f32, 5, 4, 8, 64, ks, tune="cv_splits=2,cv_tapr=0",
               expect=(("splits", 2),),
               bst=2, det=True),
        ]
    return out


def numerics_cases():
    out = []
    for f32 in (False, True):
        t = _t(f32)
        out += [
            _c(f"num-generic-fwd-{t}", "fwd", f32, 2, 9, 7, 128, 64, stride=2, tune="cv_splits=1", expect=GEN0,
               stats=True),
            _c(f"num-generic-dgrad-{t}", "dgrad", f32, 2, 5, 7, 64, 128, tune="cv_tapr=0,cv_splits=1", expect=GEN1,
               res=True),
            _c(f"num-parity-{t}", "dgrad", f32, 2, 9, 7, 64, 128, stride=2, expect=(("mode", 3),), res=True),
            _c(f"num-tapr-{t}", "fwd", f32, 2, 8, 8, 128, 64, expect=(("kind", "tapr_rows"),), stats=True),
            _c(f"num-halo-{t}", "fwd", f32, 3, 7, 7, 128, 64, expect=(("kind", "tapr_halo"),), stats=True),
            _c(f"num-splitk-{t}", "fwd", f32, 3, 7, 7, 128, 64, tune="cv_tapr=0,cv_splits=4", expect=(("splits",
                                                                                                       4),),
                                                                                                       stats=True),
        ]
    return out


EXACT_TABLES = dict(generic=generic_cases(), mode2=mode2_cases(), parity=parity_cases(), tapr=tapr_cases(),
                    halo=halo_cases(), halo_off=halo_cases(off=True), splitk=splitk_cases(), plain=plain_cases(),
                    det=det_cases())
ALL_EXACT = [c for tab in EXACT_TABLES.values() for c in tab]
NUMERICS = numerics_cases()


def ids(cases):
    return [c.id for c in cases]


# ---------------------------------------------------------------------------- wrong variants
def gather_fwd(x, w, stride, pad, bug=None, drop=None):
    """The forward conv as the kernel walks it (per tap: flat pixel index, bounds test, one GEMM),
    float64 NHWC, with one deliberate mistake: ``bug`` = "neighbour_row" (a column past the row's
    end is not padding: flat index +-1 lands in the neighbouring row), "prev_image" (a row past
    the image is read from the neighbouring image); ``drop`` = (pixel, tap): the first 16-byte
    chunk (``drop[2]`` channels) of that tap of that output pixel is skipped."""
    n, ic, H, W = x.shape
    oc, _, R, S = w.shape
    oh, ow = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    xf = nhwc(x.double()).reshape(-1, ic)
    b, i, j = torch.meshgrid(torch.arange(n), torch.arange(oh), torch.arange(ow), indexing="ij")
    y = torch.zeros(n * oh * ow, oc, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            ih, iw = (i * stride - pad + r).reshape(-1), (j * stride - pad + s).reshape(-1)
            okh, okw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
            flat = b.reshape(-1) * H * W + ih * W + iw
            ok = (okh | (bug == "prev_image")) & (okw | (bug == "neighbour_row")) & (flat >= 0) & (flat < n * H * W)
            g = xf[flat.clamp(0, n * H * W - 1)] * ok.unsqueeze(1)
            if drop is not None and drop[1] == r * S + s:
                g[drop[0], :drop[2]] = 0
            y += g @ w[:, :, r, s].double().t()
    return y.view(n, oh, ow, oc)


def gather_dgrad(dy, w, hw, pad, swap=False):
    """The stride-2 data gradient as the parity classes walk it: dx(2i+py, 2j+px) takes the taps r
    with (py + pad - r) even from dy row i + ((py + pad - r) >> 1). ``swap``: the class of a pixel
    is taken as (px, py)."""
    n, oc, P, Q = dy.shape
    ic, R, S = w.shape[1], w.shape[2], w.shape[3]
    H, W = hw
    dyf = nhwc(dy.double()).reshape(-1, oc)
    b, h, x = (t.reshape(-1) for t in torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij"))
    py, px = ((x & 1), (h & 1)) if swap else ((h & 1), (x & 1))
    dx = torch.zeros(n * H * W, ic, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            ok = (((py + pad - r) & 1) == 0) & (((px + pad - s) & 1) == 0)
            ih, iw = (h >> 1) + ((py + pad - r) >> 1), (x >> 1) + ((px + pad - s) >> 1)
            ok = ok & (ih >= 0) & (ih < P) & (iw >= 0) & (iw < Q)
            flat = (b * P * Q + ih * Q + iw).clamp(0, n * P * Q - 1)
            dx += (dyf[flat] * ok.unsqueeze(1)) @ w[:, :, r, s].double()
    return dx.view(n, H, W, ic)


def _targets():
    B = False  # bf16: the statistics variants need rounding
    P3 = (("mode", 3),)
    return {
        "neighbour_row": _c("w-nrow", "fwd", True, 2, 5, 7, 32, 64, tune="cv_tapr=0"),
        "prev_image": _c("w-pimg", "fwd", True, 2, 5, 7, 32, 64, tune="cv_tapr=0"),
        "chunk_dropped": _c("w-chunk", "fwd", True, 2, 5, 7, 32, 64, tune="cv_tapr=0"),
        "last_tile_dropped": _c("w-tile", "fwd", True, 3, 5, 5, 32, 64, k=1, pad=0),
        "parity_swapped": _c("w-swap", "dgrad", True, 2, 9, 7, 64, 64, stride=2, expect=P3),
        "class_size_floor": _c("w-floor", "dgrad", True, 2, 9, 7, 64, 64, stride=2, expect=P3),
        "odd_pixels_unwritten": _c("w-odd", "dgrad", True, 2, 9, 7, 64, 64, k=1, stride=2, pad=0, expect=P3, res=True),
        "residual_per_split": _c("w-rsplit", "dgrad", True, 3, 11, 1, 64, 32, tune="cv_splits=2,cv_tapr=0", res=True),
        "fold_all_classes": _c("w-fold", "dgrad_sc", True, 2, 9, 7, 64, 64, stride=2, expect=P3),
        "stats_unrounded": _c("w-unr", "fwd", B, 3, 5, 5, 64, 64, k=1, pad=0, stats=True),
        "sshift_ignored": _c("w-shift", "fwd", B, 3, 5, 5, 64, 64, k=1, pad=0, stats=True, sshift=True),
        "mask_ge": _c("w-ge", "dgrad", B, 3, 5, 5, 64, 64, k=1, pad=0, bst=2),
        "pixels_past_npix": _c("w-past", "fwd", B, 3, 5, 5, 64, 64, k=1, pad=0, stats=True),
    }


WRONG_CONV = _targets()


def wrong_variant(name, d):
    """What a kernel with the mistake ``name`` would produce on the case data ``d``: (output or
    None, slots or None), float64, NaN where it would leave an element unwritten."""
    c, path = d["case"], d["path"]
    out = slots = None
    if name in ("neighbour_row", "prev_image"):
        out = gather_fwd(d["act"], d["w"], c.stride, c.pad, bug=name)
    elif name == "chunk_dropped":
        out = gather_fwd(d["act"], d["w"], c.stride, c.pad, drop=(17, 4, c.epc))
    elif name == "last_tile_dropped":
        out = d["ref"].clone().reshape(-1, c.out_shape[-1])
        out[out.shape[0] // path["bn"] * path["bn"]:] = float("nan")
    elif name == "parity_swapped":
        out = gather_dgrad(d["act"], d["w"], (c.h, c.w), c.pad, swap=True)
    elif name == "class_size_floor":
        out = d["ref"].clone()
        if c.h & 1:
            out[:, c.h - 1] = float("nan")
        if c.w & 1:
            out[:, :, c.w - 1] = float("nan")
    elif name == "odd_pixels_unwritten":
        out = d["ref"].clone()
        out[:, 1::2] = float("nan")
        out[:, :, 1::2] = float("nan")
    elif name == "residual_per_split":
        out = d["ref"] + (path["splits"] - 1) * d["res"]
    elif name == "fold_all_classes":
        oh, ow = c.ohw
        t = nhwc(d["dy_sc"]).reshape(-1, c.oc) @ d["w_sc"][:, :, 0, 0]
        t = t.view(c.n, oh, ow, c.ic)
        out = dgrad_reference(d["act"], d["w"], (c.h, c.w), c.stride, c.pad)
        for py in range(2):
            for px in range(2):
                sub = out[:, py::2, px::2]
                sub += t[:, :sub.shape[1], :sub.shape[2]]
    elif name == "stats_unrounded":
        slots = fwd_stats_reference(d["ref"], d["rows"], d["sshift"])
    elif name == "sshift_ignored":
        slots = fwd_stats_reference(d["stored"], d["rows"], None)
    elif name == "mask_ge":
        slots = bwd_sums_reference(d["stored"], d["rows"], d["o"], d["y1"], d["saved1"], ge=True)
    elif name == "pixels_past_npix":  # the rows past npix of the last tile stand in as the tile's first pixel
        C = c.out_shape[-1]
        st = d["stored"].reshape(-1, C)
        bn = path["bn"]
        first = st.shape[0] // bn * bn
        extra = -st.shape[0] % bn
        st2 = torch.cat([st, st[first:first + 1].expand(extra, C)])
        rows2 = torch.cat([d["rows"], d["rows"][-1:].expand(extra)])
        slots = fwd_stats_reference(st2, rows2, d["sshift"])
    else:
        raise KeyError(name)
    return out, slots


# ---------------------------------------------------------------------------- CPU tests
def test_references_match_a_naive_loop_nest():
    gen = torch.Generator().manual_seed(5)
    for stride, pad, k, hw in ((1, 1, 3, (4, 3)), (2, 1, 3, (5, 4)), (2, 0, 1, (3, 4)), (2, 3, 7, (6, 5))):
        x, w = _ints(gen, (2, 2, *hw), 3), _ints(gen, (3, 2, k, k), 2)
        assert torch.equal(fwd_reference(x, w, stride, pad), naive_fwd(x, w, stride, pad))
        oh, ow = (hw[0] + 2 * pad - k) // stride + 1, (hw[1] + 2 * pad - k) // stride + 1
        dy = _ints(gen, (2, 3, oh, ow), 3)
        assert torch.equal(dgrad_reference(dy, w, hw, stride, pad), naive_dgrad(dy, w, hw, stride, pad))
        assert torch.equal(gather_fwd(x, w, stride, pad), naive_fwd(x, w, stride, pad))
        if stride == 2:
            assert torch.equal(gather_dgrad(dy, w, hw, pad), naive_dgrad(dy, w, hw, stride, pad))
    dy2, w2 = _ints(gen, (2, 3, 3, 2), 3), _ints(gen, (3, 2, 1, 1), 2)
    x, w = _ints(gen, (2, 3, 3, 2), 3), _ints(gen, (3, 2, 3, 3), 2)
    res = _ints(gen, (2, 5, 4, 2), 4)
    want = naive_dgrad(x, w, (5, 4), 2, 1) + naive_dgrad(dy2, w2, (5, 4), 2, 0) + res
    assert torch.equal(dgrad_reference(x, w, (5, 4), 2, 1, res, dy2, w2), want)


def test_host_operand_layouts():
    w = torch.arange(2 * 8 * 9, dtype=torch.float64).view(2, 8, 3, 3)
    wf, wd = build_wf(w, 64), build_wd(w, 64)
    assert wf.shape == (2, 128) and wd.shape == (8, 64)
    for oc, c, r, s in ((0, 0, 0, 0), (1, 7, 2, 1), (1, 3, 1, 2)):
        assert wf[oc, (r * 3 + s) * 8 + c] == w[oc, c, r, s] == wd[c, (r * 3 + s) * 2 + oc]
    assert not wf[:, 72:].any() and not wd[:, 18:].any()


def test_case_ids_are_unique():
    names = ids(ALL_EXACT + NUMERICS)
    assert len(names) == len(set(names))


DOCUMENTED = [  # plans that the comments of plan_for / tapr_bn state
    (("fwd", 128, 32, 32, 64, 64, 3, 1, 1, 576, False), "", dict(kind="tapr_rows", bn=128, bm=64, wgm=2, splits=1)),
    (("fwd", 128, 32, 32, 64, 64, 3, 1, 1, 576, True), "", dict(kind="tapr_rows", bn=128, wgm=2, kps=18)),
    (("fwd", 128, 4, 4, 512, 512, 3, 1, 1, 4608, False), "", dict(kind="tapr_rows", bn=64)),
    (("fwd", 8, 7, 7, 512, 512, 3, 1, 1, 4608, False), "", dict(kind="tapr_halo", bn=64, bm=64, pix_tiles=7)),
    (("dgrad", 8, 7, 7, 512, 512, 3, 1, 1, 4608, False), "", dict(kind="tapr_halo", mode=1)),
    (("fwd", 128, 4, 4, 512, 512, 3, 1, 1, 4608, False), "cv_tapr=0", dict(kind="generic", mode=0, bm=64, bn=64,
                                                                           splits=2, kps=36)),
    (("fwd", 128, 32, 32, 64, 64, 3, 1, 1, 576, False), "cv_tapr=0", dict(kind="generic", bm=64, bn=128, splits=1,
                                                                          kps=9)),
    (("dgrad", 128, 32, 32, 64, 128, 3, 2, 1, 1152, False), "", dict(kind="generic", mode=3, splits=1)),
    (("dgrad", 2, 9, 7, 64, 8, 3, 2, 1, 128, False), "", dict(kind="generic", mode=2)),
    (("fwd", 8, 56, 56, 64, 256, 1, 1, 0, 64, False), "", dict(kind="generic", mode=0, bm=64, bn=128, kps=1)),
    (("fwd", 8, 56, 56, 64, 64, 3, 1, 1, 576, False), "cv_tapr_halo=0", dict(kind="generic")),
]


@pytest.mark.parametrize("args,tune,want", DOCUMENTED,
                         ids=[f"{a[0]}-{a[1]}x{a[2]}x{a[4]}-{'f32' if a[-1] else 'bf16'}-{t}"
                                                           for a, t, _ in DOCUMENTED])
def test_path_query_on_documented_shapes(args, tune, want, monkeypatch):
    from psx.ops import kernels as K
    monkeypatch.setenv("PSX_TUNE", tune) if tune else monkeypatch.delenv("PSX_TUNE", raising=False)
    got = K.conv2_path(*args)
    assert isinstance(got, dict) and {k: got[k] for k in want} == want, got


def test_path_query_refusals(monkeypatch):
    from psx.ops import kernels as K
    monkeypatch.delenv("PSX_TUNE", raising=False)
    assert K.conv2_path("fwd", 2, 5, 5, 48, 64, 3, 1, 1, 448, False) == -2        # IC no power of two
    assert K.conv2_path("fwd", 2, 5, 5, 64, 96, 3, 1, 1, 576, False) == -2        # OC % 64
    assert K.conv2_path("dgrad", 2, 9, 9, 64, 64, 3, 3, 1, 576, False) == -4      # stride 3
    assert K.conv2_path("dgrad_sc", 2, 9, 7, 64, 64, 1, 2, 0, 64, False) == -11   # not 3x3 / s2 / p1
    assert K.conv2_path("dgrad_sc", 2, 9, 7, 64, 32, 3, 2, 1, 320, False) == -11  # forward OC below 64: no parity path
    assert K.conv2_path("dgrad_sc", 2, 9, 7, 64, 64, 3, 2, 1, 576, False)["mode"] == 3


@pytest.mark.parametrize("case", ALL_EXACT, ids=ids(ALL_EXACT))
def test_exact_cases_meet_their_conditions(case, monkeypatch):
    """Every exact case reaches the path it names and satisfies the exactness conditions, the bf16
    statistics cases rounding in every channel among them (all asserted inside build_case);
    torch's own fp32 CPU conv reproduces the float64 reference of the forward cases bit for bit."""
    path = query_path(case, monkeypatch)
    d = case_data(case, path)
    if case.dir == "fwd":
        y32 = nhwc(F.conv2d(d["act"].float(), d["w"].float(), stride=case.stride, padding=case.pad))
        assert torch.equal(y32.double(), d["ref"])


@pytest.mark.parametrize("case", NUMERICS, ids=ids(NUMERICS))
def test_torch_fp32_lies_inside_the_numerics_bound(case, monkeypatch):
    path = query_path(case, monkeypatch)
    d = case_data(case, path, numerics=True)
    if case.dir == "fwd":
        y = nhwc(F.conv2d(d["act"].float(), d["w"].float(), stride=case.stride, padding=case.pad))
    else:
        y = nhwc(torch.nn.grad.conv2d_input((case.n, case.ic, case.h, case.w), d["w"].float(), d["act"].float(),
                                            stride=case.stride, padding=case.pad))
        if d["res"] is not None:
            y = y + d["res"].float()
    y = y.to(case.dtype)
    assert bool(within(y, d["ref"], d["bound"]).all()), case.id
    assert float(((y.double() - d["ref"]).abs() / d["bound"].clamp_min(1e-300)).max()) < 1.0


def _numerics_twin(c):
    """The numerics case of a wrong variant's target: the same launch with IC 128-deep 3x3-like
    random operands would change its path, so the target's own geometry is kept."""
    return replace(c, id=c.id + "-num")


@pytest.mark.parametrize("name", list(WRONG_CONV), ids=list(WRONG_CONV))
def test_wrong_variants_are_caught(name, monkeypatch):
    """Each deliberately wrong kernel differs from the exact reference in at least one element on
    its target case, and leaves the numerics bound on the same launch with random operands."""
    case = WRONG_CONV[name]
    path = query_path(case, monkeypatch)
    d = case_data(case, path)
    out, slots = wrong_variant(name, d)
    if out is not None:
        want = d["stored"].double().reshape(out.shape)
        got = out.float().to(case.dtype).double()
        assert bool((got != want).any()), name
    else:
        key = "bsums_ref" if case.bst else "stats_ref"
        assert bool((slots.float().double() != d[key]).any()), name
    dn = case_data(_numerics_twin(case), path, numerics=True)
    out, slots = wrong_variant(name, dn)
    if out is not None:
        assert not bool(within(out.reshape(dn["ref"].shape), dn["ref"], dn["bound"]).all()), name
    else:
        key = "bsums_ref" if case.bst else "stats_ref"
        tot, ref = slots.sum(0), dn[key].sum(0)
        assert not bool(within(tot, ref, slot_total_bound(dn, key)).all()), name


def slot_total_bound(d, key, stored=None):
    """Any-order fp32 bound of a slot total over all P pixels, built as the element bound: every
    term rounds at most 3 times and passes at most P adds, (P + 3) 2u sum |term| [NS][C].
    ``stored``: the tensor the sums are of (default: the reference's)."""
    c = d["case"]
    C = c.out_shape[-1]
    stored = d["stored"] if stored is None else stored
    if key == "stats_ref":
        dd = stored.double().reshape(-1, C) - (d["sshift"].double() if d.get("sshift") is not None else 0.0)
        mags = torch.stack([dd.abs().sum(0), (dd * dd).sum(0)])
    else:
        mags = bwd_terms(stored, d["o"], d["y1"], d["saved1"], d["y2"], d["saved2"]).abs().sum(1)
    P = d["rows"].numel()
    return (P + 3) * 2 * U * mags
