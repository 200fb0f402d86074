"""The SGD server kernels of csrc/kernels/optim.hip, directly: sgd_apply, sgd_apply_multi,
grad_aggregate, the fp16 pack / unpack and gather_f32, against the fp64 reference and the bound of
tests/test_sgd_cpu.py or against exact rounding, on every dispatch path. Every buffer a kernel
sees lies inside a larger allocation filled with canary values, at a chosen element offset from a
256-byte boundary; every run checks the canaries and that the wires are unchanged.

Which test reaches which branch (fp64 = within the bound of the fp64 reference):

  psx_sgd_apply
    sgd_apply_h8_kernel<IMG=0/1>      fp16 wire, no momentum, n >= 8, p 32-byte and wire / image
                                      16-byte aligned: test_matches_fp64[apply-1-float16-plain /
                                      gscale / wd] placement "aligned", n in 8, 9, 255, 2053 (every
                                      tail length); second grid-stride trip: test_grid_stride_wrap
                                      [vector_apply_wd]; image bits: test_image_rounding_edges
    falls back when                   p + 1 and p + 4 elements (p % 32), wire + 1 (g % 16),
                                      img + 1 (img % 16), n in 1, 7 (n < 8), momentum: the same
                                      test, the other placements / sizes / variants
    sgd_apply_kernel<fp16, MOM=0>     those fallbacks; second trip: test_grid_stride_wrap
                                      [scalar_apply_fp16_misaligned]
    sgd_apply_kernel<fp16, MOM=1>     test_matches_fp64[apply-1-float16-mom_first / mom / mom_wd]
    sgd_apply_kernel<fp32, MOM=0>     test_matches_fp64[apply-1-float32-plain / gscale / wd]
    sgd_apply_kernel<fp32, MOM=1>     test_matches_fp64[apply-1-float32-mom*]; second trip:
                                      test_grid_stride_wrap[scalar_apply_fp32_mom_wd]
  psx_sgd_apply_multi
    nsrc < 1, nsrc > 32               test_argument_checks
    sgd_apply_multi_h8_kernel<0/1>    fp16 wires, no momentum, wd == 0, n >= 8, all aligned:
                                      test_matches_fp64[multi-W-float16-plain / gscale], W in 1, 2,
                                      7, 32; second trip: test_grid_stride_wrap[vector_multi]
    falls back when                   as above, any one wire misaligned (the last), and wd != 0
                                      (variant wd on the aligned placement)
    sgd_apply_multi_kernel<fp16, 0>   those fallbacks; second trip: test_grid_stride_wrap
                                      [scalar_multi_fp16_misaligned]
    sgd_apply_multi_kernel<fp16, 1>   test_matches_fp64[multi-W-float16-mom*]
    sgd_apply_multi_kernel<fp32, 0/1> test_matches_fp64[multi-W-float32-*]; second trip:
                                      test_grid_stride_wrap[scalar_multi_fp32_mom_wd]
  psx_grad_aggregate
    aggregate_kernel<fp16|fp32, fp32> test_grad_aggregate, accumulate off and on (fp64); second
                                      trip: n = 1,048,576 + 77
    aggregate_kernel<fp16|fp32, fp16> the same test: the rounding to fp16 of the fp32 result
  psx_fp16_pack / psx_fp16_unpack     test_fp16_pack_rounding, test_fp16_unpack_exact (exact)
  psx_gather_f32                      test_gather_f32 (exact; second trip: n = 1,048,576 + 3)

Path agreement (test_paths_agree_*) is bit for bit: the same update through the vector kernel, the
scalar kernel, the single-wire and the multi-wire entry ends in the same bits (sgd_tail.hpp)."""
import ctypes as C

import pytest
import torch

from psx.ops import kernels as K
from psx.ops._lib import ptr, stream_ptr

from .test_lars_cpu import f32
from .test_sgd_cpu import LR, U, assert_within, sgd_inputs, sgd_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64  # canary elements on either side, at least
FILL = {torch.float32: 7.0, torch.float16: 1.0, torch.bfloat16: 3.0, torch.int64: -1}
F16, F32, BF16 = torch.float16, torch.float32, torch.bfloat16
INVALID = 1  # hipErrorInvalidValue


def bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_same_bits(a, b, what=""):
    ne = bits(a.cpu()) != bits(b.cpu())
    assert not bool(ne.any()), (what, "elements that differ:", int(ne.sum()), "of", ne.numel(),
                                "first at", int(ne.nonzero()[0]))


class Placed:
    """``x`` on the device inside a larger allocation of canaries, its first element ``off``
    elements past a 256-byte boundary."""

    def __init__(self, x, off=0, fill=None):
        es, n = x.element_size(), x.numel()
        per = 256 // es
        lead = per * -(-PAD // per)  # whole 256-byte units of canaries in front
        self.fill = FILL[x.dtype] if fill is None else fill
        self.big = torch.full((n + lead + per + off + PAD,), self.fill, dtype=x.dtype, device=DEV)
        a = ((-self.big.data_ptr()) % 256) // es  # first element on a 256-byte boundary
        self.s, self.n = a + lead + off, n
        assert self.s >= PAD and self.big.numel() - self.s - n >= PAD
        self.view = self.big[self.s:self.s + n]
        self.orig = x.to(DEV)
        self.view.copy_(self.orig)
        assert (self.view.data_ptr() - off * es) % 256 == 0

    def intact(self):
        lo, hi = self.big[:self.s], self.big[self.s + self.n:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())

    def unchanged(self):
        return torch.equal(bits(self.view), bits(self.orig))


def hp(gscale=1.0, momentum=0.0, wd=0.0, first=False, lr=LR):
    return dict(gscale=gscale, momentum=momentum, wd=wd, first=first, lr=lr)


VARIANTS = {"plain": hp(), "gscale": hp(gscale=1 / 3), "wd": hp(gscale=0.25, wd=5e-4),
            "mom_first": hp(gscale=1 / 7, momentum=0.9, first=True), "mom": hp(momentum=0.9),
            "mom_wd": hp(gscale=1 / 3, momentum=0.9, wd=5e-4)}
# element offsets from the 256-byte boundary; "wire" moves the last wire only
PLACEMENTS = {"aligned": {}, "p+1": {"p": 1}, "p+4": {"p": 4}, "wire+1": {"wire": 1}, "img+1": {"img": 1}}
NS = (1, 7, 8, 9, 255, 2053)
N_AGREE = 2053


def run(entry, p, buf, wires, h, place="aligned", img_on=False):
    """One update on placed buffers; ``buf`` None: no buffer passed. Checks the canaries and the
    wires, returns the CPU copies of p, buf and img."""
    off = PLACEMENTS[place]
    n = p.numel()
    P = Placed(p, off.get("p", 0))
    B = Placed(buf, off.get("p", 0), fill=5.0) if buf is not None else None
    img = Placed(torch.zeros(n, dtype=BF16), off.get("img", 0)) if img_on else None
    Ws = [Placed(w, off.get("wire", 0) if k == len(wires) - 1 else 0) for k, w in enumerate(wires)]
    kw = dict(gscale=h["gscale"], momentum=h["momentum"], wd=h["wd"], first=h["first"],
              buf=B.view if B else None, img=img.view if img else None)
    if entry == "apply":
        assert len(Ws) == 1
        K.sgd_apply(P.view, Ws[0].view, h["lr"], **kw)
    else:
        K.sgd_apply_multi(P.view, [w.view for w in Ws], h["lr"], **kw)
    torch.cuda.synchronize()
    assert all(x.intact() for x in [P, B, img] + Ws if x is not None), ("canaries", entry, n, place)
    assert all(w.unchanged() for w in Ws), ("wires written", entry, n, place)
    return {"p": P.view.cpu(), "buf": B.view.cpu() if B else None, "img": img.view.cpu() if img else None}


def check_fp64(out, p, buf, wires, h, what):
    p_ref, v_ref, pb, vb = sgd_reference(p, wires, buf, h["lr"], h["gscale"], h["momentum"], h["wd"], h["first"])
    assert_within(out["p"], p_ref, pb, ("p",) + what)
    if v_ref is not None:
        assert_within(out["buf"], v_ref, vb, ("buf",) + what)
    if out["img"] is not None:
        assert_same_bits(out["img"], out["p"].bfloat16(), ("img",) + what)


# ---------------------------------------------------------------------------- 1. fp64
CASES = [("apply", 1), ("multi", 1), ("multi", 2), ("multi", 7), ("multi", 32)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", [F16, F32], ids=["float16", "float32"])
@pytest.mark.parametrize("entry,W", CASES)
def test_matches_fp64(entry, W, dtype, variant):
    """p and the momentum buffer within their bounds of the fp64 reference, the image bit-equal to
    the bf16 of the p the kernel wrote, and the image changing no bit of p or the buffer; every
    size (both sides of n >= 8, every tail length) at every placement."""
    h = VARIANTS[variant]
    for n in NS:
        p, buf, gs = sgd_inputs(n, W)
        wires = [g.to(dtype) for g in gs]
        b = buf if h["momentum"] else None
        for place in PLACEMENTS:
            outs = {}
            for img_on in (False, True):
                if place == "img+1" and not img_on:
                    continue
                out = run(entry, p, b, wires, h, place, img_on)
                check_fp64(out, p, b, wires, h, (entry, W, dtype, variant, n, place, img_on))
                outs[img_on] = out
            if len(outs) == 2:
                assert_same_bits(outs[0]["p"], outs[1]["p"], ("image changed p", n, place))
                if b is not None:
                    assert_same_bits(outs[0]["buf"], outs[1]["buf"], ("image changed buf", n, place))


# ---------------------------------------------------------------------------- 2. path agreement
VECTOR_VARIANTS = {"plain": hp(), "gscale": hp(gscale=1 / 3), "wd": hp(wd=5e-4), "gscale_wd": hp(gscale=1 / 3, wd=5e-4)}


@pytest.mark.parametrize("variant", list(VECTOR_VARIANTS))
@pytest.mark.parametrize("entry,W", [("apply", 1), ("multi", 1), ("multi", 3)])
def test_paths_agree_aligned_vs_misaligned(entry, W, variant):
    """An fp16 push without momentum ends in the same bits whether its slice of the arena is
    aligned (vector kernel where there is one) or not (scalar kernel), image included."""
    h = VECTOR_VARIANTS[variant]
    p, _, gs = sgd_inputs(N_AGREE, W)
    wires = [g.half() for g in gs]
    base = run(entry, p, None, wires, h, "aligned", True)
    for place in list(PLACEMENTS)[1:]:
        out = run(entry, p, None, wires, h, place, True)
        assert_same_bits(out["p"], base["p"], ("p", entry, W, variant, place))
        assert_same_bits(out["img"], base["img"], ("img", entry, W, variant, place))


ALL_VARIANTS = dict(VARIANTS, wd_only=hp(wd=5e-4), gscale_wd=hp(gscale=1 / 3, wd=5e-4))


@pytest.mark.parametrize("variant", list(ALL_VARIANTS))
@pytest.mark.parametrize("dtype", [F16, F32], ids=["float16", "float32"])
def test_paths_agree_single_vs_multi(dtype, variant):
    """sgd_apply(p, g) and sgd_apply_multi(p, [g]): same bits in p and the buffer, on the aligned
    and on a misaligned placement."""
    h = ALL_VARIANTS[variant]
    p, buf, gs = sgd_inputs(N_AGREE, 1)
    wires = [gs[0].to(dtype)]
    b = buf if h["momentum"] else None
    outs = [run(entry, p, b, wires, h, place, True) for entry in ("apply", "multi") for place in ("aligned", "p+1")]
    for k, out in enumerate(outs[1:]):
        assert_same_bits(out["p"], outs[0]["p"], ("p", dtype, variant, k + 1))
        assert_same_bits(out["img"], outs[0]["img"], ("img", dtype, variant, k + 1))
        if b is not None:
            assert_same_bits(out["buf"], outs[0]["buf"], ("buf", dtype, variant, k + 1))


@pytest.mark.parametrize("variant", list(ALL_VARIANTS))
@pytest.mark.parametrize("W", [3, 7])
def test_paths_agree_dense_sum_vs_wires(W, variant):
    """The loopback-against-gathered contract of sgd_tail.hpp: sgd_apply on the fp32 sum formed by
    chained adds in list order against sgd_apply_multi on the W fp16 wires."""
    h = ALL_VARIANTS[variant]
    p, buf, gs = sgd_inputs(N_AGREE, W)
    wires = [g.half() for g in gs]
    dense = wires[0].float()
    for w in wires[1:]:
        dense = dense + w.float()
    b = buf if h["momentum"] else None
    for place in ("aligned", "p+1"):
        a = run("apply", p, b, [dense], h, place, True)
        m = run("multi", p, b, wires, h, place, True)
        assert_same_bits(a["p"], m["p"], ("p", W, variant, place))
        assert_same_bits(a["img"], m["img"], ("img", W, variant, place))
        if b is not None:
            assert_same_bits(a["buf"], m["buf"], ("buf", W, variant, place))


# ---------------------------------------------------------------------------- 3. grid-stride wrap
N_SCALAR_WRAP = 1048576 + 259           # > 4096 blocks x 256 threads
N_VECTOR_WRAP = 8 * 1048576 + 8 * 37 + 5  # > 4096 x 256 lanes x 8 elements, tail of 5
WRAP = {
    "scalar_apply_fp32_mom_wd": ("apply", 1, F32, VARIANTS["mom_wd"], "aligned", N_SCALAR_WRAP),
    "scalar_multi_fp32_mom_wd": ("multi", 2, F32, VARIANTS["mom_wd"], "aligned", N_SCALAR_WRAP),
    "scalar_apply_fp16_misaligned": ("apply", 1, F16, VARIANTS["gscale"], "wire+1", N_SCALAR_WRAP),
    "scalar_multi_fp16_misaligned": ("multi", 2, F16, VARIANTS["gscale"], "wire+1", N_SCALAR_WRAP),
    "vector_apply_wd": ("apply", 1, F16, VARIANTS["wd"], "aligned", N_VECTOR_WRAP),
    "vector_multi": ("multi", 2, F16, VARIANTS["gscale"], "aligned", N_VECTOR_WRAP),
}


@pytest.mark.parametrize("case", list(WRAP))
def test_grid_stride_wrap(case):
    """Sizes at which a lane takes a second trip of the grid-stride loop (the grid is capped at
    4096 blocks): the parameter counts of the real models are above them."""
    entry, W, dtype, h, place, n = WRAP[case]
    p, buf, gs = sgd_inputs(n, W)
    wires = [g.to(dtype) for g in gs]
    b = buf if h["momentum"] else None
    out = run(entry, p, b, wires, h, place, True)
    check_fp64(out, p, b, wires, h, (case,))


# ---------------------------------------------------------------------------- 4. momentum buffer
@pytest.mark.parametrize("dtype", [F16, F32], ids=["float16", "float32"])
@pytest.mark.parametrize("entry,W", [("apply", 1), ("multi", 3)])
def test_momentum_buffer_discipline(entry, W, dtype):
    """first = True does not read the buffer (a NaN buffer gives a finite result within the
    bound); momentum = 0 with a buffer passed leaves the buffer's bits alone, on the vector and
    on the scalar path."""
    p, buf, gs = sgd_inputs(N_AGREE, W)
    wires = [g.to(dtype) for g in gs]
    nan_buf = torch.full_like(buf, float("nan"))
    for variant in ("mom_first", "mom_wd"):
        h = dict(VARIANTS[variant], first=True)
        for place in ("aligned", "p+1"):
            out = run(entry, p, nan_buf, wires, h, place, True)
            assert bool(torch.isfinite(out["p"]).all()) and bool(torch.isfinite(out["buf"]).all())
            check_fp64(out, p, nan_buf, wires, h, (entry, dtype, variant, place))
    for variant in ("plain", "wd"):
        for place in ("aligned", "p+1"):
            for keep in (buf, nan_buf):
                out = run(entry, p, keep, wires, VARIANTS[variant], place, True)
                assert_same_bits(out["buf"], keep, ("buffer written without momentum", variant, place))
                check_fp64(out, p, None, wires, VARIANTS[variant], (entry, dtype, variant, place))


# ---------------------------------------------------------------------------- 5. non-finite values
@pytest.mark.parametrize("dtype", [F16, F32], ids=["float16", "float32"])
@pytest.mark.parametrize("entry,W", [("apply", 1), ("multi", 3)])
def test_non_finite_values_stay_local(entry, W, dtype):
    """inf, -inf and NaN in one wire, at every slot of a vector chunk, in the tail, first and last:
    exactly those elements of p are non-finite, every other one keeps the bits of the clean run."""
    n = N_AGREE
    p, _, gs = sgd_inputs(n, W)
    wires = [g.to(dtype) for g in gs]
    pos = [0] + [8 * (10 + 3 * j) + j for j in range(8)] + [8 * 200 + j for j in range(8)] + list(range(n - 5, n))
    assert len(set(pos)) == len(pos) and n - 1 in pos and n & 7 == 5
    vals = [float("inf"), float("-inf"), float("nan")]
    bad = wires[W // 2].clone()
    mask = torch.zeros(n, dtype=torch.bool)
    for k, i in enumerate(pos):
        bad[i] = vals[k % 3]
        mask[i] = True
    dirty = wires[:W // 2] + [bad] + wires[W // 2 + 1:]
    for variant in ("gscale", "wd"):
        h = VARIANTS[variant]
        for place in ("aligned", "p+1"):
            clean = run(entry, p, None, wires, h, place, True)
            out = run(entry, p, None, dirty, h, place, True)
            assert torch.equal(~torch.isfinite(out["p"]), mask), (entry, dtype, variant, place)
            assert_same_bits(out["p"][~mask], clean["p"][~mask], ("p", entry, dtype, variant, place))
            assert_same_bits(out["img"][~mask], clean["img"][~mask], ("img", entry, dtype, variant, place))
            nan = torch.isnan(out["p"])
            assert bool(torch.isnan(out["img"].float()[nan]).all())
            assert_same_bits(out["img"][~nan], out["p"].bfloat16()[~nan], ("img inf", entry, dtype, variant, place))


# ---------------------------------------------------------------------------- 6. edge values
def _f32_from_bits(words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(torch.float32)


# fp32 bit patterns of p' and what their bf16 image has to do
EDGE_WORDS = [
    0x3F808000,  # tie, even neighbour below: rounds down
    0x3F818000,  # tie, odd below: rounds up
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # just below / above those ties
    0x7F7FFFFF,  # the largest fp32: its image is inf
    0x7F7F8000,  # tie between the largest bf16 and inf: inf
    0x7F7F7FFF,  # just below: the largest bf16
    0x00000000,  # zero
    0x00800000, 0x00808000,  # the smallest normal, and a tie above it
    # bf16-subnormal magnitudes (fp32 subnormals): ties of both parities, their neighbours, exact
    # values, the largest (rounds up into the normal range) and the smallest (rounds to zero)
    0x00008000, 0x00018000, 0x00007FFF, 0x00008001, 0x00017FFF, 0x00018001, 0x00010000, 0x007F0000, 0x007FFFFF,
    0x00000001,
]
EDGE_NAN_WORDS = [0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF]  # quiet, signalling (low bit only), negative


@pytest.mark.parametrize("entry", ["apply", "multi"])
def test_image_rounding_edges(entry):
    """A zero gradient leaves p' = p exactly, so the weights are the values the image rounds: the
    vector path's image bits (pack_bf2) equal the scalar path's (f2bf), and both equal
    torch.bfloat16 rounding (to nearest, ties to even, fp32 subnormals rounded like any other
    value, overflow to inf) for every non-NaN value; a NaN stays a NaN. Every value sits at every
    slot 0..7 of a vector chunk, and seven of them in the tail."""
    vals = _f32_from_bits(EDGE_WORDS + [w | 0x80000000 for w in EDGE_WORDS] + EDGE_NAN_WORDS)
    L = vals.numel()
    n = 64 * L + 7
    p = torch.full((n,), 1.0)
    for j in range(L):
        for s in range(8):
            p[(8 * j + s) * 8 + s] = vals[j]
    p[64 * L:] = vals[torch.tensor([0, 1, 6, 12, 13, 20, L - 1])]
    nan = torch.isnan(p)
    assert int(nan.sum()) == 8 * len(EDGE_NAN_WORDS) + 1
    want = p.bfloat16()
    for zero, negative in ((0.0, False), (-0.0, True)):
        outs = {}
        for place in ("aligned", "p+1", "img+1"):
            out = run(entry, p, None, [torch.full((n,), zero, dtype=F16)], VARIANTS["gscale"], place, True)
            keep = ~nan & (p != 0) if negative else ~nan  # -0 - lr * (-0) is +0: there a zero's sign may turn
            assert_same_bits(out["p"][keep], p[keep], ("p' != p", entry, zero, place))
            assert bool(torch.isnan(out["p"][nan]).all()) and bool(torch.isnan(out["img"].float()[nan]).all())
            assert_same_bits(out["img"][~nan], out["p"].bfloat16()[~nan], ("img vs torch", entry, zero, place))
            assert_same_bits(out["img"][keep], want[keep], ("img vs expected", entry, zero, place))
            outs[place] = out
        for place in ("p+1", "img+1"):
            assert_same_bits(outs[place]["img"][~nan], outs["aligned"]["img"][~nan], ("vector vs scalar", place))
            assert_same_bits(outs[place]["p"][~nan], outs["aligned"]["p"][~nan], ("vector vs scalar p", place))
    big = want[~nan].float().abs()
    assert bool(torch.isinf(big).any()) and bool((big == 0).any())  # the edge values do reach inf and zero


@pytest.mark.parametrize("entry", ["apply", "multi"])
def test_fp16_decode_edges(entry):
    """fp16 subnormals (all of them), +-65504 and +-0 on the wire. With p = 0, lr = gscale = 1 the
    update is exact, p' = -g, so the decode is checked bit for bit; with ordinary
    hyper-parameters (half of the weights zero, where a flushed subnormal would show) p' is
    within the bound. Vector and scalar path."""
    pat = list(range(0x0001, 0x0400)) + list(range(0x8001, 0x8400)) + [0x7BFF, 0xFBFF, 0x0000, 0x8000]
    g = torch.tensor([w - (1 << 16) if w >= 1 << 15 else w for w in pat], dtype=torch.int16).view(F16)
    n = g.numel()
    assert n & 7 and float(g.float().abs().max()) == 65504.0
    zero = torch.zeros(n)
    exact = zero - g.float()
    p_mixed = sgd_inputs(n, 1)[0].clone()
    p_mixed[::2] = 0
    for place in ("aligned", "p+1", "wire+1"):
        out = run(entry, zero, None, [g], hp(lr=1.0), place, True)
        assert_same_bits(out["p"], exact, ("decode", entry, place))
        assert_same_bits(out["img"], exact.bfloat16(), ("decode img", entry, place))
        for variant in ("gscale", "wd"):
            out = run(entry, p_mixed, None, [g], VARIANTS[variant], place, True)
            check_fp64(out, p_mixed, None, [g], VARIANTS[variant], (entry, variant, place))


# ---------------------------------------------------------------------------- 7. argument checks
def test_argument_checks():
    """Through the C ABI: nsrc = 0 and nsrc = 33 return hipErrorInvalidValue and write nothing;
    n = 0 is a no-op for both entries."""
    lib = K.kernels()
    n = 255
    p, buf, gs = sgd_inputs(n, 1)
    P, B, G = Placed(p), Placed(buf, fill=5.0), Placed(gs[0].half())
    img = Placed(torch.zeros(n, dtype=BF16))
    one = (C.c_void_p * 1)(G.view.data_ptr())
    many = (C.c_void_p * 33)(*([G.view.data_ptr()] * 33))

    def multi(srcs, nsrc, n):
        return lib.psx_sgd_apply_multi(ptr(P.view), srcs, nsrc, ptr(B.view), n, LR, 1.0, 0.9, 5e-4, 0, 1,
                                       ptr(img.view), stream_ptr())

    def single(n):
        return lib.psx_sgd_apply(ptr(P.view), ptr(G.view), ptr(B.view), n, LR, 1.0, 0.9, 5e-4, 0, 1, ptr(img.view),
                                 stream_ptr())

    assert [multi(one, 0, n), multi(many, 33, n), multi(one, -1, n)] == [INVALID] * 3
    assert [multi(one, 1, 0), single(0)] == [0, 0]
    torch.cuda.synchronize()
    for x in (P, B, G, img):
        assert x.unchanged() and x.intact()
    assert multi(many, 32, n) == 0 and single(n) == 0  # the same calls with good arguments run
    torch.cuda.synchronize()
    assert not P.unchanged() and not B.unchanged() and not img.unchanged() and G.unchanged()
    assert all(x.intact() for x in (P, B, G, img))
    with pytest.raises(AssertionError):
        K.sgd_apply_multi(P.view, [], LR)
    with pytest.raises(AssertionError):
        K.sgd_apply_multi(P.view, [G.view] * 33, LR)


# ---------------------------------------------------------------------------- 8. grad_aggregate
AGG_NS = (1, 255, 100003, 1048576 + 77)


def _agg_sources(dtype):
    """32 sources of the largest size, order 1, on the device (fp32 or their fp16 rounding);
    element 0 is large enough for a sum beyond the fp16 range."""
    if dtype not in _agg_sources.cache:
        gen = torch.Generator().manual_seed(99)
        base = torch.randn(32, AGG_NS[-1], generator=gen)
        base[:, 0] = 7e4 if dtype == F32 else 65504.0
        _agg_sources.cache[dtype] = base.to(dtype)
    return _agg_sources.cache[dtype]


_agg_sources.cache = {}


@pytest.mark.parametrize("nsrc", [1, 3, 32])
@pytest.mark.parametrize("src_dtype", [F16, F32], ids=["float16", "float32"])
def test_grad_aggregate(src_dtype, nsrc):
    """dst = scale * sum_k src_k [+ dst], all four type pairs, accumulate off and on. The fp32
    destination within 2u ((nsrc + 2) scale sum |src| + |dst_old| + |result|) of fp64 (nsrc - 1
    adds, the scaling, the accumulate add). The fp16 destination bit-equal to the fp16 rounding of
    the fp32 destination's result from the same call with dst_old.float() as the base; a sum
    beyond 65504 becomes inf. Without accumulate the destination is not read (it holds NaN)."""
    scale = 1.0 / nsrc
    gen = torch.Generator().manual_seed(5)
    for n in AGG_NS:
        cpu = _agg_sources(src_dtype)[:nsrc, :n]
        srcs = [Placed(cpu[k]) for k in range(nsrc)]
        table = torch.tensor([s.view.data_ptr() for s in srcs], dtype=torch.int64, device=DEV)
        old16 = torch.randn(n, generator=gen).half()
        old16[0] = 65504.0
        ssum = torch.zeros(n, dtype=torch.float64)
        sabs = torch.zeros(n, dtype=torch.float64)
        for k in range(nsrc):
            ssum += cpu[k].double()
            sabs += cpu[k].double().abs()
        for acc in (False, True):
            res = {}
            for dt in (F32, F16):
                start = old16.to(dt) if acc else torch.full((n,), float("nan"), dtype=dt)
                D = Placed(start, fill=9.0)
                K.grad_aggregate(table, nsrc, src_dtype == F16, D.view, n, scale=scale, accumulate=acc)
                torch.cuda.synchronize()
                what = (src_dtype, dt, nsrc, n, acc)
                assert D.intact() and all(s.intact() and s.unchanged() for s in srcs), what
                res[dt] = D.view.cpu()
            ref = ssum * f32(scale) + (old16.double() if acc else 0.0)
            bound = 2 * U * ((nsrc + 2) * f32(scale) * sabs + (old16.double().abs() if acc else 0.0) + ref.abs())
            assert_within(res[F32], ref, bound, what)
            assert_same_bits(res[F16], res[F32].half(), what)
            if acc or src_dtype == F32:
                assert bool(torch.isinf(res[F16][0])) and bool(torch.isfinite(res[F32][0])), what
            assert bool(torch.isfinite(res[F16][1:]).all())


# ---------------------------------------------------------------------------- 9. codec, gather
def _pack_inputs():
    """fp32 values around everything fp16 rounding can do: every finite fp16 value, every midpoint
    of two neighbours (a tie) and its fp32 neighbours on either side, both signs; the overflow
    threshold, values that round to inf, to the smallest subnormal and to zero, +-0, inf, NaN."""
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(F16).float()
    pos = every[torch.isfinite(every) & (every >= 0)].unique()  # sorted
    mid = (pos[:-1] + pos[1:]) / 2
    assert bool((mid.double() == (pos[:-1].double() + pos[1:].double()) / 2).all())  # exact in fp32
    inf = torch.tensor(float("inf"))
    near = torch.cat([mid, torch.nextafter(mid, -inf), torch.nextafter(mid, inf)])
    extra = torch.tensor([65520.0, 65519.996, 65520.004, 65536.0, 1e5, 3e38, 2.0 ** -25, 2.0 ** -26, 1e-30,
                          float("inf")])
    extra = torch.cat([extra, torch.nextafter(torch.tensor([2.0 ** -25]), inf)])
    x = torch.cat([every[torch.isfinite(every)], near, -near, extra, -extra, torch.tensor([float("nan")])])
    return x


@pytest.mark.parametrize("scale", [1.0, 0.5, 1 / 3])
def test_fp16_pack_rounding(scale):
    """fp16_pack = the fp32 product src * scale rounded to nearest even fp16, bit for bit (NaN:
    NaN): what the CPU codec's (g * scale).half() gives. A multiply fused into the conversion
    (v_fma_mixlo_f16) rounds the exact product once instead: with scale = 1/3 that differed on
    1016 of these inputs (fp32 products on an fp16 tie), and with every scale it turned -0 into
    +0."""
    x = _pack_inputs()
    want = (x * torch.tensor(scale, dtype=F32)).half()
    if scale == 1.0:  # the construction reaches both directions of a tie, inf and zero
        assert bool(torch.isinf(want[x.abs() == 65520.0]).all()) and bool((want[x.abs() == 2.0 ** -25] == 0).all())
    S, D = Placed(x), Placed(torch.zeros(x.numel(), dtype=F16))
    K.fp16_pack(S.view, D.view, scale)
    torch.cuda.synchronize()
    assert S.intact() and S.unchanged() and D.intact()
    got = D.view.cpu()
    nan = torch.isnan(x)
    assert bool(torch.isnan(got[nan]).all())
    assert_same_bits(got[~nan], want[~nan], ("fp16_pack", scale))


@pytest.mark.parametrize("scale", [1.0, 0.5, 1 / 3, 2.0])
def test_fp16_unpack_exact(scale):
    """fp16_unpack decodes every one of the 65,536 fp16 bit patterns exactly and multiplies by
    scale in fp32."""
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(F16)
    want = every.float() * torch.tensor(scale, dtype=F32)
    S, D = Placed(every), Placed(torch.zeros(65536))
    K.fp16_unpack(S.view, D.view, scale)
    torch.cuda.synchronize()
    assert S.intact() and S.unchanged() and D.intact()
    got = D.view.cpu()
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2 * 1023 and bool(torch.isnan(got[nan]).all())
    assert_same_bits(got[~nan], want[~nan], ("fp16_unpack", scale))


@pytest.mark.parametrize("n", [1, 1000, 1048576 + 3])
def test_gather_f32(n):
    """dst[i] = src[idx[i]] bit for bit: random int64 indices with repeats, index 0 and the last."""
    m = 4099 if n <= 1000 else 2 * 1048576 + 5
    gen = torch.Generator().manual_seed(n)
    src = torch.randn(m, generator=gen)
    idx = torch.randint(0, m, (n,), generator=gen, dtype=torch.int64)
    idx[0] = 0
    idx[-1] = m - 1
    assert n == 1 or idx.unique().numel() < n
    S, I, D = Placed(src), Placed(idx), Placed(torch.full((n,), float("nan")))
    K.gather_f32(S.view, I.view, D.view)
    torch.cuda.synchronize()
    assert all(x.intact() for x in (S, I, D)) and S.unchanged() and I.unchanged()
    assert_same_bits(D.view.cpu(), src[idx], ("gather_f32", n))
