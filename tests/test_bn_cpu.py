"""The fp64 references of the BatchNorm kernels (csrc/kernels/bn.hip, csrc/kernels/bnfin.hpp), the
error bounds the kernels are held to, a host mirror of the deterministic mode's fixed-point
encoder, and the CPU tests that give the bounds their meaning: every plain fp32 evaluation of a
formula stays inside its bound and every wrong formula (WRONG_STATS, WRONG_BWD, the wrong
applies) leaves it, on the inputs
the GPU tests use. Everything public here is shared with tests/test_bn_gpu.py.

Conventions. Activations are [npix, C] (NHWC with the pixels flattened); bf16 tensors decode
exactly; hyper-parameters are rounded to fp32 first. Every reference returns float64 tensors and
one bound per output element. The bounds are first order in u = 2^-24 (plus the rounding of a bf16
or fp16 sink), one term per rounding the kernel performs, absolute in the magnitudes of the
operands (an element that cancels is held to the same bound as its neighbours), and doubled for
the second-order terms and for fused multiply-adds, which only remove roundings."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from psx.ops.kernels import det_slot_values

from .test_lars_cpu import f32
from .test_sgd_cpu import U, assert_within, within

U_BF16 = 2.0 ** -9   # bf16 sink: doubled with the rest it is 2^-8, the unit roundoff of bf16 (8 significant
                     # bits), so round-to-nearest just fits and a truncating store (up to 2^-7) does not
U_F16 = 2.0 ** -11   # of fp16; below 2^-14 its spacing is 2^-24, so a sink adds 2^-25 absolutely
U64 = 2.0 ** -50     # allowance for the kernels' float64 work (a few roundings of 2^-53)
SLOTS = 8            # PSX_STAT_SLOTS
EPS, MOMENTUM = 1e-5, 0.1
BF16, F32 = torch.bfloat16, torch.float32


def sink_rounding(dtype):
    return {torch.float32: 0.0, torch.bfloat16: U_BF16, torch.float16: U_F16}[dtype]


# ---------------------------------------------------------------------------- fixed point
POISON = 1 << 63
M64 = (1 << 64) - 1


def fix_encode(v):
    """Host mirror of fix_add (bnfin.hpp): the pair (hi, lo) of unsigned 64-bit words that the
    fp32 partial ``v`` adds to its slot entry, hi = floor(v 2^24) (two's complement) and lo =
    trunc(frac(v 2^24) 2^40), computed with the same float64 operations; a partial that is not
    finite or not below 2^38 in magnitude adds nothing and sets bit 63 of the low word instead:
    (0, POISON), to be OR-ed (FixAcc)."""
    v = float(np.float32(v))
    if not abs(v) < 274877906944.0:  # false for NaN too
        return 0, POISON
    x = v * 16777216.0
    h = math.floor(x)
    lo = int((x - h) * 1099511627776.0)
    return int(h) & M64, lo


class FixAcc:
    """One slot entry: the two 64-bit words under wrapping integer adds (atomicAdd) and the sticky
    poison bit (atomicOr)."""

    def __init__(self):
        self.hi = self.lo = 0

    def add(self, v):
        hi, lo = fix_encode(v)
        if lo & POISON:
            self.lo |= POISON
        else:
            self.hi = (self.hi + hi) & M64
            self.lo = (self.lo + lo) & M64
        return self

    def words(self):
        return self.hi, self.lo

    def exact(self):
        """The value the words stand for, as a Fraction (None when poisoned)."""
        if self.lo & POISON:
            return None
        hi = self.hi - (1 << 64) if self.hi >> 63 else self.hi
        return Fraction(hi, 1 << 24) + Fraction(self.lo, 1 << 64)

    def pair(self):
        """The words as the int64 pair of the slot buffer."""
        s = lambda w: w - (1 << 64) if w >> 63 else w
        return torch.tensor([s(self.hi), s(self.lo)], dtype=torch.int64)


def fix_encode_tensor(v):
    """fix_encode of every element of the fp32 tensor ``v``: int64 [..., 2] and the poison mask."""
    v = v.float().double()
    bad = ~(v.abs() < 274877906944.0)
    x = torch.where(bad, torch.zeros_like(v), v) * 16777216.0
    h = torch.floor(x)
    lo = ((x - h) * 1099511627776.0).to(torch.int64)  # truncates, as the kernel's conversion
    return torch.stack([h.to(torch.int64), lo], -1), bad


def det_slots(partials, nrows=SLOTS):
    """The deterministic-mode slot pairs [nrows, ..., 2] (int64) after the fp32 ``partials``
    [W, ...] were added, partial w to slot row w % nrows: wrapping integer sums and the sticky
    poison bit, whatever the order."""
    W = partials.shape[0]
    rows = [w % nrows for w in range(W)]
    out = torch.zeros((nrows,) + tuple(partials.shape[1:]) + (2,), dtype=torch.int64)
    for w in range(W):
        pair, bad = fix_encode_tensor(partials[w])
        pair = torch.where(bad.unsqueeze(-1), torch.zeros_like(pair), pair)
        out[rows[w]] += pair
        out[rows[w], ..., 1] |= torch.where(bad, torch.tensor(-2 ** 63), torch.tensor(0))
    return out


def det_buffer(pairs):
    """The pairs as the fp32 slot buffer a kernel is handed (entry i at byte 16 i: four times the
    float layout)."""
    return pairs.contiguous().view(torch.float32).reshape(-1)


def det_total(pairs):
    """Sum over the slot rows of int64 pairs [T, ..., 2] as the consumers take it: the integer
    sums of both words, converted once. float64 [...]; NaN where any row is poisoned."""
    poison = (pairs[..., 1] < 0).any(0)
    H = pairs[..., 0].sum(0)
    L = (pairs[..., 1] & (2 ** 63 - 1)).sum(0)
    v = H.double() * 2.0 ** -24 + L.double() * 2.0 ** -64
    return torch.where(poison, torch.full_like(v, float("nan")), v)


def slot_total(slots, det=False, fp32_depth=0):
    """(sum over the slot rows, its bound). ``slots``: the fp32 rows [T, ...], summed in float64 as
    the folded finalizes do (bound: the float64 allowance); the standalone finalize kernels first
    add ``fp32_depth`` = ceil(T / 8) rows in fp32 (0 + x exact, so depth - 1 roundings; depth u
    sum |rows| holds them). ``det``: int64 pairs [T, ..., 2], integer sums: exact up to the one
    conversion."""
    if det:
        tot = det_total(slots)
        mag = (slots[..., 0].double().abs() * 2.0 ** -24).sum(0) + 1.0
        return tot, U64 * mag
    d = slots.double()
    return d.sum(0), (fp32_depth * U + U64) * d.abs().sum(0)


# ---------------------------------------------------------------------------- launch geometry
def reduce_geometry(npix, C):
    """bn_bwd_reduce's launch (psx_bn_bwd_reduce): ppb pixels per workgroup, wgs workgroups, tpp
    threads sharing a channel group; a thread adds per_thread terms, LDS combines tpp partials,
    and slot row r takes the workgroups b with b % 8 == r."""
    if C % 8 or 256 % (C // 8):
        raise ValueError("bn_bwd_reduce needs C / 8 to divide 256")
    ppb = max(64, -(-npix // 512))
    wgs = -(-npix // ppb)
    tpp = 256 // (C // 8)
    return dict(ppb=ppb, wgs=wgs, tpp=tpp, per_thread=-(-ppb // tpp), per_row=-(-wgs // SLOTS))


def ew_grid(nvec, cap=2048):
    """Workgroups of an elementwise launch over nvec 8-channel vectors (cap 512 with the folded
    finalize)."""
    return max(1, min(cap, -(-nvec // 256)))


# ---------------------------------------------------------------------------- references
def bn_stats_reference(slots, count, sshift, gamma, beta, eps, momentum, run_mean, run_var, det=False,
                       fp32_depth=0, b_slots=None):
    """Forward finalize from the slot sums [T, 2, C] (row 0: sum (x - k), row 1: sum (x - k)^2, k =
    sshift or 0; ``det``: int64 pairs [T, 2, C, 2]) in float64:

        m1 = s / n;  mean = k + m1;  var = max(ss / n - m1^2, 0);  invstd = 1 / sqrt(var + eps)
        scale = gamma invstd;  shift = beta - mean scale;  saved = (mean, invstd);  sshift_next = mean
        run_mean' = (1 - m) run_mean + m mean;  run_var' = (1 - m) run_var + m var n / (n - 1)
        (the unbiased factor only when n > 1)

    Returns (ref, bound): dicts of float64 [C] under the keys mean, var, invstd, scale, shift,
    sshift_next and, with running statistics, run_mean, run_var.

    Bounds. The kernels do the moments in float64, so with b(s), b(ss) the bounds of the slot sums
    (slot_total: nothing but the float64 allowance for the folded finalizes and the deterministic
    mode, depth u sum |slot| for the standalone kernel's fp32 group sums)
      mean     b(s) / n, and one rounding to fp32: u |mean|
      var      b(ss) / n + 2 |m1| b(s) / n, and U64 (ss / n + m1^2) for the float64 subtraction
      invstd   the image of [var - b, var + b] under 1 / sqrt(max(., 0) + eps) (not linearised:
               var may be 0), and one rounding: u invstd
      scale    |gamma| b(invstd), one product: u |scale|
      shift    |scale| b(mean) + |mean| b(scale), the product and the subtraction:
               u (|mean scale| + |shift|)   (|shift| <= |beta| + |mean scale|: absolute)
      run_mean the rounding of 1 - m, two products, one add: u (2 |(1 - m) run_mean| + |m mean| +
               |run_mean'|), and m b(mean)
      run_var  likewise with unb = var n / (n - 1) rounded to fp32: m (b(var) n / (n - 1) + u unb)
    each doubled. ``b_slots`` [2, C] (the chain test): what the slot sums themselves may be off
    the quantity the caller compares with, added to b(s), b(ss)."""
    eps, momentum, n = f32(eps), f32(momentum), f32(count)
    tot, btot = slot_total(slots, det, fp32_depth)
    if b_slots is not None:
        btot = btot + b_slots
    s, ss, bs, bss = tot[0], tot[1], btot[0], btot[1]
    k = sshift.double() if sshift is not None else torch.zeros_like(s)
    gamma, beta = gamma.double(), beta.double()
    m1 = s / n
    mean = k + m1
    raw = ss / n - m1 * m1
    var = raw.clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    b_mean = bs / n + U * mean.abs()
    b_var = bss / n + 2 * m1.abs() * bs / n + U64 * (ss.abs() / n + m1 * m1)
    hi = 1.0 / torch.sqrt((var - b_var).clamp_min(0.0) + eps)
    lo = 1.0 / torch.sqrt(var + b_var + eps)
    b_is = (hi - lo) + U * invstd
    b_scale = gamma.abs() * b_is + U * scale.abs()
    b_shift = scale.abs() * b_mean + mean.abs() * b_scale + U * ((mean * scale).abs() + beta.abs() + (mean * scale).abs())
    ref = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, sshift_next=mean)
    bound = dict(mean=2 * b_mean, var=2 * b_var, invstd=2 * b_is, scale=2 * b_scale, shift=2 * b_shift,
                 sshift_next=2 * b_mean)
    if run_mean is not None:
        rm, rv = run_mean.double(), run_var.double()
        unb = var * n / (n - 1.0) if n > 1.0 else var
        b_unb = (b_var * n / (n - 1.0) if n > 1.0 else b_var) + U * unb
        ref["run_mean"] = (1.0 - momentum) * rm + momentum * mean
        ref["run_var"] = (1.0 - momentum) * rv + momentum * unb
        bound["run_mean"] = 2 * (U * (2 * ((1.0 - momentum) * rm).abs() + (momentum * mean).abs()
                                      + ((1.0 - momentum) * rm).abs() + (momentum * mean).abs()) + momentum * b_mean)
        bound["run_var"] = 2 * (U * (2 * ((1.0 - momentum) * rv).abs() + momentum * unb
                                     + ((1.0 - momentum) * rv).abs() + momentum * unb) + momentum * b_unb)
    return ref, bound


def bn_eval_affine_reference(gamma, beta, rm, rv, eps, r_rsqrt):
    """Eval-mode affine: scale = gamma / sqrt(rv + eps), shift = beta - rm scale. ``r_rsqrt``: the
    relative error allowed to the kernel's rsqrtf. Roundings: rv + eps (half of it reaches the
    root: u / 2), rsqrtf, the product; then as the training shift. Doubled."""
    eps = f32(eps)
    gamma, beta, rm, rv = (t.double() for t in (gamma, beta, rm, rv))
    scale = gamma / torch.sqrt(rv + eps)
    shift = beta - rm * scale
    b_scale = scale.abs() * (U / 2 + r_rsqrt + U)
    b_shift = rm.abs() * b_scale + U * (2 * (rm * scale).abs() + beta.abs())
    return scale, shift, 2 * b_scale, 2 * b_shift


def bn_apply_reference(y, scale, shift, res, scale2, shift2, relu, mode, out_dtype=None):
    """out = act(y scale + shift [+ res] [+ res scale2 + shift2]), mode 0 / 1 / 2, from the fp32
    affine(s) the kernel used. Returns (out, bound) [npix, C].

    Bound: with A = |y scale| + |shift| (+ |res| or |res scale2| + |shift2|), every partial result
    is at most A and mode 0 / 1 / 2 rounds 2 / 3 / 5 times: roundings u A; ReLU never increases a
    difference; a bf16 sink adds 2^-9 |out|. Doubled."""
    out_dtype = out_dtype or y.dtype
    y, scale, shift = y.double(), scale.double(), shift.double()
    t = y * scale + shift
    A = (y * scale).abs() + shift.abs()
    n = 2
    if mode == 1:
        t = t + res.double()
        A = A + res.double().abs()
        n = 3
    elif mode == 2:
        t2 = res.double() * scale2.double()
        t = t + t2 + shift2.double()
        A = A + t2.abs() + shift2.double().abs()
        n = 5
    out = t.clamp_min(0.0) if relu else t
    return out, 2 * (n * U * A + sink_rounding(out_dtype) * out.abs())


def float_slots(partials, nrows=SLOTS):
    """The float-mode slot rows [nrows, ...] (fp32) holding the same partials: row r the float64
    sum of the partials w with w % nrows == r, rounded once (an input: the references sum these)."""
    out = torch.zeros((nrows,) + tuple(partials.shape[1:]), dtype=torch.float64)
    out.index_add_(0, torch.arange(partials.shape[0]) % nrows, partials.double())
    return out.float()


def slot_rows(npix, geo):
    """Slot row of every pixel under the reduce's geometry."""
    return (torch.arange(npix) // geo["ppb"]) % SLOTS


def bn_bwd_sums_reference(g, o, y1, saved1, y2=None, saved2=None, mask=True, geo=None, det=False):
    """The backward sums per slot row, float64 [SLOTS, NS, C]: sum dz, sum dz xhat1 [, sum dz
    xhat2] with dz = g [o > 0] (or g without the mask) and xhat = (y - mean) invstd from the saved
    fp32 statistics [2, C]; pixel p belongs to workgroup p // ppb and to slot row (p // ppb) % 8
    (``geo``: reduce_geometry; without it everything is in row 0). Returns (sums, bound).

    Bound of a row. A term dz (y - mean) invstd rounds three times (3 u |term|; dz itself is
    exact). Adding rounds once per add: a thread adds per_thread terms, LDS combines tpp partials,
    and the row takes per_row float atomics, so a term passes at most per_thread + tpp + per_row
    adds, each rounding a partial sum of magnitude at most A = sum |term| over the row:
        u (3 [xhat rows] + per_thread + tpp + per_row) A
    In deterministic mode everything after the workgroup partial is exact integer arithmetic
    (fix_add truncates below 2^-64 per add): the per_row term is replaced by the float64
    allowance. Doubled."""
    gd = g.double()
    dz = gd * (o.double() > 0).double() if mask else gd
    terms = [dz, dz * (y1.double() - saved1[0].double()) * saved1[1].double()]
    if y2 is not None:
        terms.append(dz * (y2.double() - saved2[0].double()) * saved2[1].double())
    npix, C = g.shape
    if geo is None:
        geo = dict(ppb=npix, per_thread=npix, tpp=1, per_row=1)
    rows = slot_rows(npix, geo)
    NS = len(terms)
    sums = torch.zeros(SLOTS, NS, C, dtype=torch.float64)
    mags = torch.zeros(SLOTS, NS, C, dtype=torch.float64)
    for k, t in enumerate(terms):
        sums[:, k].index_add_(0, rows, t)
        mags[:, k].index_add_(0, rows, t.abs())
    depth = geo["per_thread"] + geo["tpp"] + (0 if det else geo["per_row"])
    per = torch.tensor([0.0] + [3.0] * (NS - 1)).view(1, NS, 1) + depth
    extra = (U64 * mags + geo["per_row"] * 2.0 ** -64) if det else 0.0
    return sums, 2 * (U * per * mags + extra)


def bn_bwd_coef_reference(sdz, sxh, count, gamma, saved, gscale, b_sdz=None, b_sxh=None, b_mean=None, b_is=None,
                          sink=torch.float32):
    """Backward finalize from the total sums [C] (float64) and the saved fp32 statistics [2, C]:

        mdz = sdz / n;  mxh = sxh / n;  k1 = gamma is;  k2 = -gamma is^2 mxh
        k3 = -gamma is mdz + gamma is^2 mean mxh;  dgamma = sxh gscale;  dbeta = sdz gscale

    Returns (ref, bound), dicts with k1, k2, k3, dgamma, dbeta. The bounds propagate those of the
    sums (b_sdz, b_sxh) linearly and add the kernel's roundings (mdz, mxh and the sums for the
    gradients are rounded to fp32 first):
      k1      u |k1|
      k2      4 u |k2| + |gamma is^2| b_sxh / n
      k3      a = gamma is mdz: 3 u |a| + |gamma is| b_sdz / n;  b = gamma is^2 mean mxh: 5 u |b| +
              |gamma is^2 mean| b_sxh / n;  the add: u (|a| + |b|)
      dgamma  2 u |dgamma| + gscale b_sxh, plus the sink's rounding (fp16: 2^-11 |dgamma| + 2^-25)
    b_mean, b_is (the chain test): the statistics themselves are only known within these, which
    moves k1 by |gamma| b_is, k2 by 2 |gamma is mxh| b_is, k3 by |gamma mdz| b_is + |gamma mxh|
    (2 |is mean| b_is + is^2 b_mean). Doubled."""
    n, gscale = f32(count), f32(gscale)
    gm, mean, is_ = gamma.double(), saved[0].double(), saved[1].double()
    z = torch.zeros_like(sdz)
    b_sdz = z if b_sdz is None else b_sdz
    b_sxh = z if b_sxh is None else b_sxh
    b_mean = z if b_mean is None else b_mean
    b_is = z if b_is is None else b_is
    mdz, mxh = sdz / n, sxh / n
    k1 = gm * is_
    k2 = -gm * is_ * is_ * mxh
    a, b = gm * is_ * mdz, gm * is_ * is_ * mean * mxh
    k3 = -a + b
    dg, db = sxh * gscale, sdz * gscale
    sr = sink_rounding(sink)
    tiny = 2.0 ** -25 if sink == torch.float16 else 0.0
    bound = dict(
        k1=2 * (U * k1.abs() + gm.abs() * b_is),
        k2=2 * (4 * U * k2.abs() + (gm * is_ * is_).abs() * b_sxh / n + 2 * (gm * is_ * mxh).abs() * b_is),
        k3=2 * (3 * U * a.abs() + (gm * is_).abs() * b_sdz / n + 5 * U * b.abs()
                + (gm * is_ * is_ * mean).abs() * b_sxh / n + U * (a.abs() + b.abs())
                + (gm * mdz).abs() * b_is + (gm * mxh).abs() * (2 * (is_ * mean).abs() * b_is + is_ * is_ * b_mean)),
        dgamma=2 * ((2 * U + sr) * dg.abs() + gscale * b_sxh + tiny),
        dbeta=2 * ((2 * U + sr) * db.abs() + gscale * b_sdz + tiny))
    return dict(k1=k1, k2=k2, k3=k3, dgamma=dg, dbeta=db), bound


def bn_bwd_apply_reference(g, o, y, coef, mask=True, b_coef=None, out_dtype=None):
    """dx = k1 dz + k2 y + k3 with dz = g [o > 0] (or g), ``coef`` = (k1, k2, k3) [C] each.
    Returns (dx, dz, bound). The apply rounds two products and two adds, every partial result at
    most A = |k1 dz| + |k2 y| + |k3|: 3 u A covers them, a bf16 sink adds 2^-9 |dx|; with ``b_coef``
    = (b(k1), b(k2), b(k3)), the coefficients' own bounds, the whole chain is
    |dz| b(k1) + |y| b(k2) + b(k3) on top. The apply's part is doubled (b_coef already is)."""
    out_dtype = out_dtype or g.dtype
    k1, k2, k3 = (c.double() for c in coef)
    gd, yd = g.double(), y.double()
    dz = gd * (o.double() > 0).double() if mask else gd
    dx = k1 * dz + k2 * yd + k3
    A = (k1 * dz).abs() + (k2 * yd).abs() + k3.abs()
    bound = 2 * (3 * U * A + sink_rounding(out_dtype) * dx.abs())
    if b_coef is not None:
        bound = bound + dz.abs() * b_coef[0] + yd.abs() * b_coef[1] + b_coef[2]
    return dx, dz, bound


# ---------------------------------------------------------------------------- inputs
def bn_params(C, seed=0):
    """Per-channel parameters, all distinct: gamma in [0.5, 1.5) with gamma[1] negative and
    gamma[2] zero, beta in [-0.3, 0.3), running statistics, a second set for the shortcut BN."""
    ch = torch.arange(C, dtype=torch.float32)
    out = {}
    for tag, r in (("", 0), ("2", 3)):
        gamma = 0.5 + ((ch + r) % C) / C
        gamma[1], gamma[2] = -0.75 - 0.01 * r, 0.0
        out["gamma" + tag] = gamma
        out["beta" + tag] = -0.3 + 0.6 * (((ch + r) * 3) % C) / C + 0.001 * ch / C
        out["run_mean" + tag] = 0.2 - 0.4 * ch / C
        out["run_var" + tag] = 0.8 + 0.5 * ((ch * 5 + r) % C) / C + 0.001 * ch / C
    return out


def bn_inputs(C, npix, dtype=F32, big_mean=False, seed=0):
    """Activations y1, y2 [npix, C] (per-channel means and spreads all distinct; ``big_mean``: mean
    100 + small, std 1), a gradient g of mixed signs, and o: a true ReLU output, about half of it
    exact +0 and five elements -0.0. Cached: the tests share them and leave them unchanged."""
    key = (C, npix, dtype, big_mean, seed)
    if key not in bn_inputs.cache:
        gen = torch.Generator().manual_seed(977 + 13 * seed + C + npix % 1013)
        ch = torch.arange(C, dtype=torch.float32)
        base = 100.0 if big_mean else 0.0
        mu1, mu2 = base + 0.25 + 0.5 * ch / C, base - 0.2 - 0.4 * ch / C
        sd1 = torch.ones(C) if big_mean else 0.5 + 1.5 * ((ch * 7) % C) / C
        sd2 = torch.ones(C) if big_mean else 0.6 + 1.2 * ((ch * 3 + 1) % C) / C
        y1 = (mu1 + sd1 * torch.randn(npix, C, generator=gen)).to(dtype)
        y2 = (mu2 + sd2 * torch.randn(npix, C, generator=gen)).to(dtype)
        g = torch.randn(npix, C, generator=gen).to(dtype)
        o = torch.randn(npix, C, generator=gen).clamp_min(0.0).to(dtype)
        flat = o.view(-1)
        zeros = (flat == 0).nonzero().view(-1)
        flat[zeros[:: max(1, zeros.numel() // 5)][:5]] = -0.0
        bn_inputs.cache[key] = dict(y1=y1, y2=y2, g=g, o=o)
    return bn_inputs.cache[key]


bn_inputs.cache = {}


def true_saved(y):
    """fp32 saved statistics [2, C] of an activation (mean, invstd), as a forward would leave."""
    yd = y.double()
    mean = yd.mean(0)
    var = (yd * yd).mean(0) - mean * mean
    return torch.stack([mean, 1.0 / torch.sqrt(var.clamp_min(0) + f32(EPS))]).float()


def stats_slots(y, T, sshift=None, nparts=None):
    """Host-built forward partials [W, 2, C] (fp32) of an activation: pixel p goes to partial
    p % W (W = nparts or T), each the float64 sum of (y - k), (y - k)^2 rounded to fp32 (what a
    producer's workgroup would add)."""
    W = nparts or T
    yd = y.double() - (sshift.double() if sshift is not None else 0.0)
    idx = torch.arange(y.shape[0]) % W
    part = torch.zeros(W, 2, y.shape[1], dtype=torch.float64)
    part[:, 0].index_add_(0, idx, yd)
    part[:, 1].index_add_(0, idx, yd * yd)
    return part.float()


def stats_case(C, T, kind):
    """Inputs of a forward finalize: (slots [T, 2, C] fp32, count, sshift or None). Kinds:
    ``plain``; ``count1`` (one pixel); ``big`` (mean 100 / std 1, unshifted sums); ``big_shift``
    (the same activation, sums shifted by k = the mean + 0.01). Channel 3 is the constant 0.5 (sums
    exact, variance exactly 0) and channel 4 the constant fp32(0.1) (variance rounds to either
    side of 0: the clamp)."""
    n = 1 if kind == "count1" else 5 * T + 3
    y = bn_inputs(C, n, F32, big_mean=kind.startswith("big"), seed=T)["y1"].clone()
    k = None
    if kind == "big_shift":
        k = (y.double().mean(0) + 0.01).float()
    else:
        y[:, 3], y[:, 4] = 0.5, 0.1
    return stats_slots(y, T, k), n, k


# ---------------------------------------------------------------------------- fp32 emulations
def _fma(a, b, c):
    """fp32 fused multiply-add through float64 (the product is exact there)."""
    return (a.double() * b.double() + c.double()).float()


def emulate_stats(slots, count, sshift, gamma, beta, eps, momentum, rm, rv, group_sums, reverse, fused):
    """bn_finalize in plain arithmetic: float64 moments as the kernel, fp32 affine and running
    statistics; ``group_sums``: the standalone kernel's fp32 sums of rows g, g + 8, ... first."""
    T = slots.shape[0]
    order = list(range(T))[::-1] if reverse else list(range(T))
    if group_sums:
        grp = [torch.zeros_like(slots[0]) for _ in range(8)]
        for t in order:
            grp[t % 8] = grp[t % 8] + slots[t]
        tot = sum(x.double() for x in (grp[::-1] if reverse else grp))
    else:
        tot = sum(slots[t].double() for t in order)
    n = torch.tensor(f32(count), dtype=torch.float32)
    k = sshift.double() if sshift is not None else 0.0
    m1 = tot[0] / n.double()
    mean = k + m1
    var = (tot[1] / n.double() - m1 * m1).clamp_min(0.0)
    invstd = (1.0 / torch.sqrt(var + f32(eps))).float()
    sc = gamma * invstd
    sh = _fma(-mean.float(), sc, beta) if fused else beta - mean.float() * sc
    mom = torch.tensor(f32(momentum), dtype=torch.float32)
    one_m = torch.tensor(1.0, dtype=torch.float32) - mom
    unb = (var * n.double() / (n.double() - 1.0) if f32(count) > 1 else var).float()
    if fused:
        nrm, nrv = _fma(one_m, rm, mom * mean.float()), _fma(mom, unb, one_m * rv)
    else:
        nrm, nrv = one_m * rm + mom * mean.float(), one_m * rv + mom * unb
    return dict(mean=mean.float(), invstd=invstd, scale=sc, shift=sh, sshift_next=mean.float(), run_mean=nrm,
                run_var=nrv)


def emulate_apply(y, sc, sh, res, sc2, sh2, relu, mode, fused):
    yf = y.float()
    t = _fma(yf, sc, sh) if fused else yf * sc + sh
    if mode == 1:
        t = t + res.float()
    elif mode == 2:
        t = _fma(res.float(), sc2, t) + sh2 if fused else t + (res.float() * sc2 + sh2)
    t = t.clamp_min(0.0) if relu else t
    return t.to(y.dtype)


def emulate_sums(g, o, y1, saved1, y2, saved2, mask, geo, reverse, fused):
    """bn_bwd_reduce's sums per slot row in fp32, in the kernel's order of adds (thread, LDS, slot
    atomics in workgroup order) or each stage reversed."""
    npix, C = g.shape
    d = g.float() * (o.float() > 0).float() if mask else g.float()
    ys = [(y1, saved1)] + ([(y2, saved2)] if y2 is not None else [])
    ppb, tpp, nt, wgs = geo["ppb"], geo["tpp"], geo["per_thread"], geo["wgs"]
    pad = wgs * nt * tpp  # pixel (b, k, q) = b ppb + k tpp + q, valid while k tpp + q < ppb and < npix
    b, k, q = torch.meshgrid(torch.arange(wgs), torch.arange(nt), torch.arange(tpp), indexing="ij")
    p = b * ppb + k * tpp + q
    valid = ((k * tpp + q) < ppb) & (p < npix)
    p = p.clamp_max(npix - 1)

    def lay(x):
        return torch.where(valid.unsqueeze(-1), x[p.reshape(-1)].view(wgs, nt, tpp, C), torch.zeros(()))

    rows = []
    for stat in range(1 + len(ys)):
        dd = lay(d)
        acc = torch.zeros(wgs, tpp, C)
        ks = range(nt - 1, -1, -1) if reverse else range(nt)
        for kk in ks:
            if stat == 0:
                acc = acc + dd[:, kk]
            else:
                y, sv = ys[stat - 1]
                t = dd[:, kk] * (lay(y.float())[:, kk] - sv[0])
                acc = _fma(t, sv[1].expand_as(t), acc) if fused else acc + t * sv[1]
        wg = torch.zeros(wgs, C)
        for qq in (range(tpp - 1, -1, -1) if reverse else range(tpp)):
            wg = wg + acc[:, qq]
        row = torch.zeros(SLOTS, C)
        for bb in (range(wgs - 1, -1, -1) if reverse else range(wgs)):
            row[bb % SLOTS] = row[bb % SLOTS] + wg[bb]
        rows.append(row)
    return torch.stack(rows, 1)


def emulate_coef(sdz, sxh, count, gamma, saved, gscale, fused, sink=torch.float32):
    n = f32(count)
    mdz, mxh = (sdz / n).float(), (sxh / n).float()
    gm, mean, is_ = gamma, saved[0], saved[1]
    a, b = -gm * is_ * mdz, gm * is_ * is_ * mean
    k3 = _fma(b, mxh, a) if fused else a + b * mxh
    gs = torch.tensor(f32(gscale), dtype=torch.float32)
    return dict(k1=gm * is_, k2=-gm * is_ * is_ * mxh, k3=k3, dgamma=(sxh.float() * gs).to(sink).float(),
                dbeta=(sdz.float() * gs).to(sink).float())


def emulate_bwd_apply(g, o, y, coef, mask, fused):
    d = g.float() * (o.float() > 0).float() if mask else g.float()
    k1, k2, k3 = coef
    r = _fma(k1.expand_as(d), d, _fma(k2.expand_as(d), y.float(), k3.expand_as(d))) if fused \
        else k1 * d + k2 * y.float() + k3
    return r.to(g.dtype)


# ---------------------------------------------------------------------------- shapes of the GPU tests
STATS_C, STATS_T = (8, 40, 64), (1, 8, 19)
APPLY_SHAPES = ((8, 33), (48, 33), (64, 33))
REDUCE_SHAPES = [(C, npix) for C in (8, 64, 2048) for npix in (1, 64, 65, 577)] + [(8, 32833)]
CHAIN = (64, 577)


def _check_all(got, ref, bound, keys, what):
    for key in keys:
        assert_within(got[key], ref[key], bound[key], (key,) + what)


STAT_KEYS = ("mean", "invstd", "scale", "shift", "sshift_next", "run_mean", "run_var")


# ---------------------------------------------------------------------------- CPU tests: emulations
@pytest.mark.parametrize("kind", ["plain", "count1", "big", "big_shift"])
def test_stats_emulations_stay_inside(kind):
    for C in STATS_C:
        P = bn_params(C)
        for T in ((1,) if kind == "count1" else STATS_T):
            slots, n, k = stats_case(C, T, kind)
            for group in (False, True):
                ref, bound = bn_stats_reference(slots, n, k, P["gamma"], P["beta"], EPS, MOMENTUM, P["run_mean"],
                                                P["run_var"], fp32_depth=-(-T // 8) if group else 0)
                for reverse in (False, True):
                    for fused in (False, True):
                        got = emulate_stats(slots, n, k, P["gamma"], P["beta"], EPS, MOMENTUM, P["run_mean"],
                                            P["run_var"], group, reverse, fused)
                        _check_all(got, ref, bound, STAT_KEYS, (kind, C, T, group, reverse, fused))
            if kind == "count1":
                # one pixel: the variance is the rounding of the fp32 sum of squares, and the
                # running variance takes it as it is (no n / (n - 1))
                assert bool((ref["var"] <= 2 * U * ref["mean"] ** 2).all())
                want = (1.0 - f32(MOMENTUM)) * P["run_var"].double() + f32(MOMENTUM) * ref["var"]
                assert torch.equal(ref["run_var"], want)
            elif kind != "big_shift":
                assert float(ref["var"][3]) == 0.0 and float(ref["invstd"][3]) == 1.0 / math.sqrt(f32(EPS))


def test_stats_deterministic_pairs_match_float_slots():
    """The same partials through the fixed-point pairs give the reference of their float64 sum."""
    for C, T in ((8, 1), (40, 19)):
        P = bn_params(C)
        slots, n, k = stats_case(C, T, "plain")
        ref, bound = bn_stats_reference(slots, n, k, P["gamma"], P["beta"], EPS, MOMENTUM, None, None)
        dref, dbound = bn_stats_reference(det_slots(slots), n, k, P["gamma"], P["beta"], EPS, MOMENTUM, None, None,
                                          det=True)
        _check_all(dref, ref, bound, ("mean", "invstd", "scale", "shift"), (C, T))
        assert "run_mean" not in dref and bool((dbound["shift"] <= 1.01 * bound["shift"]).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_apply_emulations_stay_inside(dtype):
    for C, npix in APPLY_SHAPES:
        x, P = bn_inputs(C, npix, dtype), bn_params(C)
        sc, sh = P["gamma"], P["beta"]
        sc2, sh2 = P["gamma2"], P["beta2"]
        for mode in (0, 1, 2):
            for relu in (False, True):
                ref, bound = bn_apply_reference(x["y1"], sc, sh, x["y2"], sc2, sh2, relu, mode)
                for fused in (False, True):
                    got = emulate_apply(x["y1"], sc, sh, x["y2"], sc2, sh2, relu, mode, fused)
                    assert_within(got, ref, bound, (dtype, C, npix, mode, relu, fused))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_backward_emulations_stay_inside(dtype):
    """Sums (kernel order and reversed, fused and not, both modes' bounds), coefficients from the
    emulated sums, and dx through the whole chain."""
    for C, npix in REDUCE_SHAPES:
        if C == 2048 and npix == 577 and dtype == BF16:
            continue  # the same geometry as fp32, 1.2 M elements: once is enough on the CPU
        x, P = bn_inputs(C, npix, dtype), bn_params(C)
        s1, s2 = true_saved(x["y1"]), true_saved(x["y2"])
        geo = reduce_geometry(npix, C)
        for det in (False, True):
            ref, bound = bn_bwd_sums_reference(x["g"], x["o"], x["y1"], s1, x["y2"], s2, True, geo, det)
            for reverse, fused in ((False, False), (True, False), (False, True)):
                got = emulate_sums(x["g"], x["o"], x["y1"], s1, x["y2"], s2, True, geo, reverse or det, fused)
                if det:  # exact after the workgroup partial: the float64 sum of the fp32 row is no worse
                    got = got.double()
                assert_within(got, ref, bound, ("sums", dtype, C, npix, det, reverse, fused))
        tot, btot = ref.sum(0), bound.sum(0)
        for which, (gm, sv, y) in enumerate(((P["gamma"], s1, x["y1"]), (P["gamma2"], s2, x["y2"])), 1):
            for gscale in (1.0, 1 / 3):
                for sink in (torch.float32, torch.float16):
                    cref, cb = bn_bwd_coef_reference(tot[0], tot[which], npix, gm, sv, gscale, btot[0], btot[which],
                                                     sink=sink)
                    gsum = got.double().sum(0)
                    for fused in (False, True):
                        c = emulate_coef(gsum[0], gsum[which], npix, gm, sv, gscale, fused, sink)
                        _check_all(c, cref, cb, ("k1", "k2", "k3", "dgamma", "dbeta"), (dtype, C, npix, which, gscale))
            coef = (c["k1"], c["k2"], c["k3"])
            dx, dz, bdx = bn_bwd_apply_reference(x["g"], x["o"], y, (cref["k1"], cref["k2"], cref["k3"]), True,
                                                 (cb["k1"], cb["k2"], cb["k3"]))
            for fused in (False, True):
                assert_within(emulate_bwd_apply(x["g"], x["o"], y, coef, True, fused), dx, bdx,
                              ("dx", dtype, C, npix, which, fused))


def test_deterministic_bound_is_tighter():
    for C, npix in REDUCE_SHAPES:
        x = bn_inputs(C, npix, F32)
        s1, geo = true_saved(x["y1"]), reduce_geometry(npix, C)
        a = bn_bwd_sums_reference(x["g"], x["o"], x["y1"], s1, geo=geo, det=False)[1]
        b = bn_bwd_sums_reference(x["g"], x["o"], x["y1"], s1, geo=geo, det=True)[1]
        used = a > 0
        assert bool((b[used] < a[used]).all()), (C, npix)


def test_reduce_geometry():
    assert reduce_geometry(577, 64) == dict(ppb=64, wgs=10, tpp=32, per_thread=2, per_row=2)
    assert reduce_geometry(32833, 8) == dict(ppb=65, wgs=506, tpp=256, per_thread=1, per_row=64)
    assert reduce_geometry(65, 2048)["tpp"] == 1 and reduce_geometry(65, 2048)["wgs"] == 2
    with pytest.raises(ValueError):
        reduce_geometry(64, 48)
    assert ew_grid(524296) == 2048 and 524296 > 2048 * 256 and ew_grid(131080, 512) == 512
    assert (512 * 256) % 6 != 0  # C 48: a thread's channel group changes between grid-stride trips


# ---------------------------------------------------------------------------- CPU tests: wrong variants
def _wrong_stats(name, slots, n, k, P):
    """The forward finalize with one mistake, in float64."""
    eps, m, n = f32(EPS), f32(MOMENTUM), float(n)
    use = slots[:-1] if name == "slot_row_dropped" else slots
    tot = use.double().sum(0)
    cnt = n - 1.0 if name == "count_minus_one" else n
    m1 = tot[0] / cnt
    mean = m1 if name == "shift_not_added" else (k.double() if k is not None else 0.0) + m1
    var = (tot[1] / cnt - m1 * m1).clamp_min(0.0)
    invstd = 1.0 / (torch.sqrt(var) + eps) if name == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
    scale = P["gamma"].double() * invstd
    unb = var if name == "biased_running_var" else var * n / (n - 1.0)
    a, b = (m, 1.0 - m) if name == "momentum_swapped" else (1.0 - m, m)
    return dict(mean=mean, invstd=invstd, scale=scale, shift=P["beta"].double() - mean * scale, sshift_next=mean,
                run_mean=a * P["run_mean"].double() + b * mean, run_var=a * P["run_var"].double() + b * unb)


WRONG_STATS = {"biased_running_var": "run_var", "eps_outside_sqrt": "invstd", "momentum_swapped": "run_mean",
               "shift_not_added": "mean", "count_minus_one": "mean", "slot_row_dropped": "mean"}


@pytest.mark.parametrize("name", ["none"] + list(WRONG_STATS))
def test_wrong_stats_leave_the_bound(name):
    """On the shifted mean-100 case and the plain one, at every C and every T > 1 of the GPU tests,
    under the looser (standalone kernel) bound."""
    for kind in ("plain", "big_shift"):
        if name == "shift_not_added" and kind == "plain":
            continue
        for C in STATS_C:
            P = bn_params(C)
            for T in STATS_T[1:]:
                slots, n, k = stats_case(C, T, kind)
                ref, bound = bn_stats_reference(slots, n, k, P["gamma"], P["beta"], EPS, MOMENTUM, P["run_mean"],
                                                P["run_var"], fp32_depth=-(-T // 8))
                got = _wrong_stats(name, slots, n, k, P)
                if name == "none":
                    _check_all(got, ref, bound, STAT_KEYS, (kind, C, T))
                    continue
                key = WRONG_STATS[name]
                bad = int((~within(got[key], ref[key], bound[key])).sum())
                assert bad > C // 2, (name, kind, C, T, key, bad)


def test_wrong_applies_leave_the_bound():
    """shift2 dropped in mode 2; the next channel group's parameters (the affine rolled by 8); and,
    beyond the list, a bf16 store that truncates instead of rounding to nearest."""
    for dtype in (F32, BF16):
        for C, npix in APPLY_SHAPES:
            x, P = bn_inputs(C, npix, dtype), bn_params(C)
            sc, sh, sc2, sh2 = P["gamma"], P["beta"], P["gamma2"], P["beta2"]
            ref, bound = bn_apply_reference(x["y1"], sc, sh, x["y2"], sc2, sh2, False, 2)
            if dtype == BF16:
                chopped = (ref.float().view(torch.int32) & -65536).view(torch.float32)
                assert int((~within(chopped, ref, bound)).sum()) > 0, C
            no_shift2 = bn_apply_reference(x["y1"], sc, sh, x["y2"], sc2, torch.zeros(C), False, 2)[0]
            assert int((~within(no_shift2, ref, bound)).sum()) > ref.numel() // 2, (dtype, C)
            if C > 8:
                for mode in (0, 1, 2):
                    nxt = bn_apply_reference(x["y1"], sc.roll(-8), sh.roll(-8), x["y2"], sc2.roll(-8), sh2.roll(-8),
                                             False, mode)[0]
                    assert int((~within(nxt, ref if mode == 2 else bn_apply_reference(
                        x["y1"], sc, sh, x["y2"], sc2, sh2, False, mode)[0], bound)).sum()) > ref.numel() // 2
                k = (P["gamma"], P["beta"], P["gamma2"])
                dx, _, b = bn_bwd_apply_reference(x["g"], x["o"], x["y1"], k)
                nxt = bn_bwd_apply_reference(x["g"], x["o"], x["y1"], tuple(t.roll(-8) for t in k))[0]
                assert int((~within(nxt, dx, b)).sum()) > dx.numel() // 2


WRONG_BWD = ("mask_ge", "pixel_dropped", "dgamma_without_invstd", "k2_sign", "k3_without_mean", "gscale_dropped",
             "count_minus_one")


@pytest.mark.parametrize("name", WRONG_BWD)
@pytest.mark.parametrize("det", [False, True], ids=["float", "det"])
def test_wrong_backward_leaves_the_bound(name, det):
    """The backward with one mistake, in float64, at every shape of the reduce's GPU test (the
    sums per slot row under that geometry's bound; the coefficients under the propagated one)."""
    for C, npix in REDUCE_SHAPES:
        if npix == 1:
            continue  # a single pixel: xhat = 0 and nothing is left to drop or to divide by
        if name == "count_minus_one" and npix > 577:
            # n - 1 moves k2 by |k2| / n = 3e-5 |k2| at n = 32,833: less than the 256 + 64 fp32 adds of
            # that geometry may lose (2 u 324 = 3.9e-5 of sum |term|). The forward's count - 1
            # (test_wrong_stats_leave_the_bound) is outside at every shape.
            continue
        x, P = bn_inputs(C, npix, F32), bn_params(C)
        s1, geo = true_saved(x["y1"]), reduce_geometry(npix, C)
        ref, bound = bn_bwd_sums_reference(x["g"], x["o"], x["y1"], s1, None, None, True, geo, det)
        g, o, sv = x["g"], x["o"], s1
        if name == "mask_ge":
            o = torch.where(o.double() >= 0, torch.ones_like(o), o)
        elif name == "pixel_dropped":
            g = g.clone()
            g[-1] = 0.0
        elif name == "dgamma_without_invstd":
            sv = torch.stack([s1[0], torch.ones(C)])
        got = bn_bwd_sums_reference(g, o, x["y1"], sv, None, None, True, geo, det)[0]
        if name in ("mask_ge", "pixel_dropped", "dgamma_without_invstd"):
            bad = int((~within(got, ref, bound)).sum())
            assert bad > 0 and (name == "pixel_dropped" or bad >= C // 2), (name, C, npix, bad)
            continue
        tot, btot = ref.sum(0), bound.sum(0)
        cref, cb = bn_bwd_coef_reference(tot[0], tot[1], npix, P["gamma"], s1, 1 / 3, btot[0], btot[1])
        n = npix - 1 if name == "count_minus_one" else npix
        c = bn_bwd_coef_reference(tot[0], tot[1], n, P["gamma"], s1, 1.0 if name == "gscale_dropped" else 1 / 3)[0]
        if name == "k2_sign":
            c["k2"] = -c["k2"]
        elif name == "k3_without_mean":
            c["k3"] = -P["gamma"].double() * s1[1].double() * tot[0] / npix
        key = {"k2_sign": "k2", "k3_without_mean": "k3", "gscale_dropped": "dgamma", "count_minus_one": "k2"}[name]
        bad = int((~within(c[key], cref[key], cb[key])).sum())
        # (n - 1 moves k2 by |k2| / n: outside only where the channel's sum is not itself small)
        assert bad >= (1 if name == "count_minus_one" else C // 2), (name, C, npix, key, bad)


# ---------------------------------------------------------------------------- CPU tests: fixed point
def _decode(acc):
    return float(det_slot_values(acc.pair(), (1,))[0])


def _close(x, exact):
    """Equal up to the decode's own float64 roundings (two conversions and one add)."""
    return abs(Fraction(x) - exact) <= Fraction(3, 1 << 53) * abs(exact)


PARTIALS = [1.0, -1.0, 0.1, -0.1, 3.5e-7, -2.25e4, 2.0 ** -41, -(2.0 ** -41), 2.0 ** 38 - 2.0 ** 14,
            -(2.0 ** 38 - 2.0 ** 14), 1234.5678, -1e-3, 2.0 ** -24, -(2.0 ** -24) * 1.5]


def test_fix_encode_is_exact_down_to_2_pow_minus_41():
    for v in PARTIALS:
        v = f32(v)
        acc = FixAcc().add(v)
        assert acc.exact() == Fraction(v), v
        assert 0 <= acc.words()[1] < 1 << 40
        assert _close(_decode(acc), Fraction(v)) or v == 0
    acc = FixAcc()
    for v in PARTIALS:
        acc.add(v)
    exact = sum(Fraction(f32(v)) for v in PARTIALS)
    assert acc.exact() == exact
    # the decoded double: the high word's conversion may round at 2^-53 of |H 2^-24| (<= 2^39)
    assert abs(Fraction(_decode(acc)) - exact) <= Fraction(3, 1 << 53) * Fraction(2 ** 39)


def test_fix_encode_truncates_below_2_pow_minus_41_by_less_than_2_pow_minus_64():
    for v in (2.0 ** -42 * 1.0000001, -(2.0 ** -42) * 1.0000001, 3e-20, -3e-20, 1.4e-45, -1.4e-45, 2.0 ** -41 * 0.75):
        v = f32(v)
        lost = Fraction(v) - FixAcc().add(v).exact()
        assert -Fraction(1, 1 << 77) <= lost < Fraction(1, 1 << 64), (v, lost)
        assert FixAcc().add(v).words() == FixAcc().add(v).words()
    acc = FixAcc()
    vs = [f32(x) for x in (3e-20, -3e-20, 1.4e-45, -7e-15, 2.5e-13)] * 3
    for v in vs:
        acc.add(v)
    lost = sum(Fraction(v) for v in vs) - acc.exact()
    assert -len(vs) * Fraction(1, 1 << 77) <= lost < len(vs) * Fraction(1, 1 << 64)


def test_fix_adds_commute():
    import itertools
    import random

    vs = [f32(v) for v in PARTIALS]
    want = None
    rnd = random.Random(5)
    for _ in range(50):
        rnd.shuffle(vs)
        acc = FixAcc()
        for v in vs:
            acc.add(v)
        want = want or acc.words()
        assert acc.words() == want
    for perm in itertools.permutations([f32(-0.1), f32(2.0 ** 37), f32(-3e-20), float("inf")]):
        acc = FixAcc()
        for v in perm:
            acc.add(v)
        assert acc.words()[1] & POISON and acc.words()[0] == FixAcc().add(-0.1).add(2.0 ** 37).add(-3e-20).words()[0]


@pytest.mark.parametrize("bad", [2.0 ** 38, -(2.0 ** 38), 1e30, float("inf"), float("-inf"), float("nan")])
def test_fix_poison(bad):
    assert fix_encode(bad) == (0, POISON)
    assert fix_encode(f32(2.0 ** 38 - 2.0 ** 14))[1] < POISON
    acc = FixAcc().add(1.0).add(bad)
    assert math.isnan(_decode(acc)) and acc.exact() is None
    for v in PARTIALS * 3:  # the poison survives later adds (low words stay far below bit 63)
        acc.add(v)
    assert acc.words()[1] & POISON and math.isnan(_decode(acc))


def test_tensor_encoder_equals_the_scalar_one():
    vs = torch.tensor(PARTIALS + [float("inf"), float("nan"), 2.0 ** 38, 3e-20, -1.4e-45], dtype=torch.float32)
    pair, bad = fix_encode_tensor(vs)
    for i, v in enumerate(vs.tolist()):
        hi, lo = fix_encode(v)
        if lo & POISON:
            assert bool(bad[i])
        else:
            assert not bool(bad[i]) and (int(pair[i, 0]) & M64, int(pair[i, 1])) == (hi, lo)
    parts = vs.view(-1, 1).repeat(1, 3)
    parts[-5:, 0] = 1.0  # column 0 stays clean
    slots = det_slots(parts)
    assert slots.shape == (SLOTS, 3, 2)
    tot = det_total(slots)
    exact = sum(Fraction(float(v)) for v in parts[:, 0].tolist())
    assert abs(Fraction(float(tot[0])) - exact) <= Fraction(3, 1 << 53) * Fraction(2 ** 39)
    assert math.isnan(float(tot[1])) and math.isnan(float(tot[2]))
    vals = det_slot_values(det_buffer(slots), (SLOTS, 3))
    assert bool(torch.isnan(vals[:, 1]).any()) and bool(torch.isfinite(vals[:, 0]).all())
    assert det_buffer(slots).numel() == 4 * SLOTS * 3
