"""The fp64 references of the implicit-GEMM weight gradient (csrc/kernels/wgrad_v2.hip, the stem's
in stem.hip) and of its split-K reduction (csrc/kernels/wgrad_reduce.hip), the operands that make a
comparison with them exact, the case tables of tests/test_wgrad_paths_gpu.py, and the CPU tests
that give all of it its meaning. Everything public here is shared with the GPU module.

Exact operands. x holds integers in [-3, 3], dy in [-2, 2]: every product and every partial sum is
an integer of magnitude at most 6 npix < 2^24, exact in fp32 in any order, on either MFMA, so every
split slab must equal the float64 reference bit for bit, and so must the reduced gradient (power-of-
two scales; the fp16 wire is one round-to-nearest-even of the exact value, as ``(_Float16)val``).
operands() asserts the conditions. Operands are built on the host as NHWC with the padded channel
count cp (channels cin .. cp-1 zero), never through another kernel.

Slabs. Slab s of a route with ``kps`` steps of ``pix`` pixels per split is the sum over the pixels
[s kps pix, min(npix, (s + 1) kps pix)) (the kernels' pbeg = split * steps_per_split * PIX); the
stem's persistent grid gives tile t (4 output rows = 448 pixels) to slab t % 256. Columns are
tap * cp + c (tap = r * S + s); columns >= R S cp are exactly 0.0.

Numerics cases (random bf16-representable operands) hold an element to
    (n + 1) 2u sum |dy||x|  [+ half an fp16 ulp of the reference on the fp16 wire]
with n the real products (the output pixels whose tap lies inside the image) plus the adds of the
splits, u = 2^-24: the bound of tests/test_conv_cpu.py, unchanged.

Instantiations. COMPILED lists the 18 kernels of wgrad_v2.hip's launch tables and the stem's;
REACHED is what the case table reaches (asserted), UNREACHED what no geometry of the planner search
in test_unreached_instantiations_stay_unreached selects: bf16 tile 128x128x4, the bf16 tap-reuse
BC 128 kernels with the 6-deep ring (both width kinds) and fp32 tile 128x128. A planner change that
starts choosing one of them fails that test until a case is added. (The four fp32 tile kernels are
also run in 1x1 form through K.bgemm_tn_f32 by the GPU module.)"""
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

from .test_bn_cpu import BF16, F32, U  # noqa: F401  (re-exported to the GPU module)
from .test_conv_cpu import ids, nhwc
from .test_sgd_cpu import within

LIM = 2.0 ** 24
F16 = torch.float16
NAN = float("nan")
SCALES = (1.0, 2.0 ** -7)
STEM_TILE, STEM_GRID = 4 * 112, 256  # stem.hip: kS7WRows output rows per tile, kS7WGrid workgroups
K_PRE = 16                           # wgrad_reduce.hip kPre


# ---------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class WCase:
    """One weight gradient. route: (kind, br, bc, ns) K.conv_wgrad2_path must report; multi: more
    than one split; short: the last split has fewer steps than the others (steps % kps != 0)."""
    id: str
    f32: bool
    n: int
    h: int
    w: int
    cp: int
    oc: int
    k: int = 3
    stride: int = 1
    pad: int = 1
    cin: int = 0
    route: tuple = ()
    multi: bool = False
    short: bool = False
    seed: int = 0

    @property
    def dtype(self):
        return F32 if self.f32 else BF16

    @property
    def ci(self):
        return self.cin or self.cp

    @property
    def ohw(self):
        return ((self.h + 2 * self.pad - self.k) // self.stride + 1,
                (self.w + 2 * self.pad - self.k) // self.stride + 1)

    @property
    def npix(self):
        return self.n * self.ohw[0] * self.ohw[1]

    @property
    def kg(self):
        return -(-(self.k * self.k * self.cp) // 64) * 64

    def args(self):
        return (self.n, self.h, self.w, self.cp, self.oc, self.k, self.stride, self.pad, self.kg, self.f32)

    @property
    def inst(self):
        return (self.route[0], self.f32) + tuple(self.route[1:])


def query_route(case):
    """K.conv_wgrad2_path of the case, checked against what the case names. Host code only."""
    from psx.ops import kernels as K
    path = K.conv_wgrad2_path(*case.args())
    assert isinstance(path, dict), (case.id, "refused", path)
    assert (path["kind"], path["br"], path["bc"], path["ns"]) == case.route and path["f32"] == case.f32, \
        (case.id, "planner took", path)
    assert (path["splits"] > 1) == case.multi, (case.id, path)
    assert path["splits"] == K.conv_wgrad2_splits(*case.args())
    if path["kind"] != "stem7":
        steps = -(-case.npix // path["pix"])
        assert (path["splits"] - 1) * path["kps"] < steps <= path["splits"] * path["kps"], (case.id, path)
        assert bool(steps % path["kps"]) == case.short, (case.id, "steps", steps, path)
    return path


# ---------------------------------------------------------------------------- operands
def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).double()


def _bf(gen, shape):
    return torch.randn(shape, generator=gen).to(BF16).double()


@lru_cache(maxsize=None)
def operands(case, numerics=False):
    """(x NCHW [n][cin][h][w], dy NCHW [n][oc][oh][ow], xp NHWC [n h w][cp] zero padded, dyf NHWC
    [npix][oc]), float64. Shared: callers leave them unchanged."""
    gen = torch.Generator().manual_seed(1000 * case.seed + 17)
    oh, ow = case.ohw
    if numerics:
        x, dy = _bf(gen, (case.n, case.ci, case.h, case.w)), _bf(gen, (case.n, case.oc, oh, ow))
    else:
        x, dy = _ints(gen, (case.n, case.ci, case.h, case.w), 3), _ints(gen, (case.n, case.oc, oh, ow), 2)
        assert 6 * case.npix < LIM, (case.id, "6 npix", 6 * case.npix)
        assert float(x.abs().max()) <= 3 and float(dy.abs().max()) <= 2
        assert case.npix < 8 or not torch.equal(x, x.flip(-1)) or case.w == 1
    xp = torch.zeros(case.n * case.h * case.w, case.cp, dtype=torch.float64)
    xp[:, :case.ci] = nhwc(x).reshape(-1, case.ci)
    return x, dy, xp, nhwc(dy).reshape(-1, case.oc)


# ---------------------------------------------------------------------------- fp64 references
BUGS_GATHER = ("rs_swapped", "hw_swapped", "pad_ignored", "stride_ignored", "tap_c_transposed")
BUGS_SPLIT = ("split_off_by_one", "last_step_dropped")
BUGS_REDUCE = ("chanpad_kept", "presum_slab_stride")


def tap_rows(case, xp, r, s, bug=None):
    """[npix][cp]: the input pixel that tap (r, s) of every output pixel reads, zero outside the
    image: the kernels' gather (pixel -> (n, oh, ow) -> (ih, iw), bounds test), one deliberate
    mistake ``bug`` of BUGS_GATHER allowed."""
    H, W, (oh, ow) = case.h, case.w, case.ohw
    if bug == "rs_swapped":
        r, s = s, r
    stride = 1 if bug == "stride_ignored" else case.stride
    pad = 0 if bug == "pad_ignored" else case.pad
    pix = torch.arange(case.npix)
    b, rem = pix // (oh * ow), pix % (oh * ow)
    i, j = (rem // oh, rem % oh) if bug == "hw_swapped" else (rem // ow, rem % ow)
    ih, iw = i * stride - pad + r, j * stride - pad + s
    ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
    flat = ((b * H + ih) * W + iw).clamp(0, case.n * H * W - 1)
    return xp[flat] * ok.unsqueeze(1)


def pixel_ranges(case, path, bug=None):
    """Per slab the list of pixel ranges [p0, p1) it sums (see the module docstring)."""
    npix = case.npix
    if path["kind"] == "stem7":
        nt = npix // STEM_TILE
        return [[(t * STEM_TILE, (t + 1) * STEM_TILE) for t in range(s, nt, STEM_GRID)] for s in range(STEM_GRID)]
    pix, out = path["pix"], []
    step = path["kps"] * pix
    for s in range(path["splits"]):
        p0, p1 = s * step, min(npix, (s + 1) * step)
        if bug == "split_off_by_one":   # every inner boundary one step late
            p0 = min(npix, p0 + pix) if s else 0
            p1 = min(npix, p1 + pix) if s + 1 < path["splits"] else npix
        if bug == "last_step_dropped":  # the partial last step of the pixels
            p1 = min(p1, npix // pix * pix)
        out.append([(p0, p1)])
    return out


def ref_slabs(case, path, numerics=False, bug=None, absolute=False):
    """The partials [splits][OC][Kg], float64. ``absolute``: of |dy| and |x| (the bound's sums)."""
    _, _, xp, dyf = operands(case, numerics)
    if absolute:
        xp, dyf = xp.abs(), dyf.abs()
    R, cp = case.k, case.cp
    ranges = pixel_ranges(case, path, bug if bug in BUGS_SPLIT else None)
    slabs = torch.zeros(len(ranges), case.oc, case.kg, dtype=torch.float64)
    for r in range(R):
        for s in range(R):
            g = tap_rows(case, xp, r, s, bug if bug in BUGS_GATHER else None)
            col = (r * R + s) * cp
            for i, rs in enumerate(ranges):
                for p0, p1 in rs:
                    if p1 > p0:
                        slabs[i, :, col:col + cp] += dyf[p0:p1].t() @ g[p0:p1]
    if bug == "tap_c_transposed":  # column c * RS + tap
        RS = R * R
        slabs[:, :, :RS * cp] = slabs[:, :, :RS * cp].reshape(-1, case.oc, RS, cp).transpose(2, 3).reshape(
            -1, case.oc, RS * cp)
    return slabs


def presum_applies(splits, oc, kg, ic, k):
    """psx_wgrad_reduce sums groups of K_PRE slabs in place first: the one-thread-per-column
    kernel's layers (R S > 49 or IC % 16) with fewer than 128 workgroups and more than 32 splits."""
    v1 = k * k > 49 or ic % 16 != 0
    return v1 and oc * kg // 256 < 128 and splits > 2 * K_PRE


def reduce_reference(slabs, cin, ic, k, scale, fp16, bug=None):
    """The reduced gradient [OC][cin][R][S] of the slabs [splits][OC][Kg] (float64; NaN allowed
    wherever the reduction must not look: padded channels and padding columns), in the wire's
    dtype: sum over the splits, (oc, tap, c) -> (oc, c, tap), the channel padding dropped, times
    ``scale``, one rounding. ``bug``: one of BUGS_REDUCE."""
    splits, oc, kg = slabs.shape
    RS = k * k
    if bug == "presum_slab_stride" and presum_applies(splits, oc, kg, ic, k):
        groups = -(-splits // K_PRE)  # the final pass walks slabs 0 .. groups-1 instead of every 16th
        walked = [slabs[j * K_PRE:(j + 1) * K_PRE].sum(0) if j % K_PRE == 0 else slabs[j] for j in range(groups)]
        tot = torch.stack(walked).sum(0)
    else:
        tot = slabs.sum(0)
    t = tot[:, :RS * ic].reshape(oc, RS, ic)
    if bug == "chanpad_kept":  # o = (oc * IC + c) * RS + tap, cut to the output's length
        out = t.transpose(1, 2).reshape(-1)[:oc * cin * RS].reshape(oc, cin, k, k)
    else:
        out = t[:, :, :cin].transpose(1, 2).reshape(oc, cin, k, k)
    out = out * scale
    return out.float().to(F16) if fp16 else out.float()


def ref_oihw(case, path, scale=1.0, fp16=False, numerics=False, bug=None):
    slabs = ref_slabs(case, path, numerics, bug)
    return reduce_reference(slabs, case.ci, case.cp, case.k, scale, fp16, bug if bug in BUGS_REDUCE else None)


def half_f16_ulp(ref):
    """Half an fp16 ulp of every (float64) reference value; 2^-25 in the subnormal range."""
    _, e = torch.frexp(ref.abs().float())
    h = torch.ldexp(torch.ones_like(ref), (e.to(torch.int32) - 12).clamp_min(-25))
    return torch.where(ref == 0, torch.zeros_like(ref), h)


def numerics_reference(case, path, scale, fp16):
    """(float64 reference [OC][cin][R][S] times scale, its element bound)."""
    slabs = ref_slabs(case, path, numerics=True)
    mags = ref_slabs(case, path, numerics=True, absolute=True)

    def oihw(t):
        return t.sum(0)[:, :case.k ** 2 * case.cp].reshape(case.oc, -1, case.cp)[:, :, :case.ci].transpose(1, 2)

    ones = torch.ones(case.n * case.h * case.w, 1, dtype=torch.float64)
    nprod = torch.tensor([float(tap_rows(case, ones, r, s).sum()) for r in range(case.k) for s in range(case.k)])
    n = nprod + (path["splits"] - 1)
    ref = (oihw(slabs) * scale).reshape(case.oc, case.ci, case.k, case.k)
    bound = ((n + 1) * 2 * U * oihw(mags) * scale).reshape(ref.shape)
    return ref, bound + (half_f16_ulp(ref) if fp16 else 0)


def naive_wgrad(x, dy, k, stride, pad):
    n, ic, H, W = x.shape
    _, oc, P, Q = dy.shape
    dw = torch.zeros(oc, ic, k, k, dtype=torch.float64)
    for b in range(n):
        for i in range(P):
            for j in range(Q):
                for r in range(k):
                    for s in range(k):
                        ih, iw = i * stride - pad + r, j * stride - pad + s
                        if 0 <= ih < H and 0 <= iw < W:
                            dw[:, :, r, s] += torch.outer(dy[b, :, i, j], x[b, :, ih, iw])
    return dw


def torch_wgrad(case, numerics=False, dtype=torch.float64):
    x, dy, _, _ = operands(case, numerics)
    return torch.nn.grad.conv2d_weight(x.to(dtype), (case.oc, case.ci, case.k, case.k), dy.to(dtype),
                                       stride=case.stride, padding=case.pad)


# ---------------------------------------------------------------------------- case tables
def _w(id, t, n, h, w, cp, oc, k, stride, pad, route, multi=False, short=False, cin=0):
    return WCase(id=id, f32=t == "f32", n=n, h=h, w=w, cp=cp, oc=oc, k=k, stride=stride, pad=pad, cin=cin,
                 route=route, multi=multi, short=short, seed=len(id) + n + h)


T64, T64W, T128 = ("tile", 64, 64, 3), ("tile", 64, 128, 3), ("tile", 128, 64, 3)
TAP3, TAP6, TAP3W = ("tap_reuse", 192, 64, 3), ("tap_reuse", 192, 64, 6), ("tap_reuse", 192, 128, 3)
GEN3, GEN6, GEN3W = (("tap_reuse_general",) + t[1:] for t in (TAP3, TAP6, TAP3W))
STEM = ("stem7", 0, 0, 0)


def route_cases():
    """Every instantiation the planner can be made to choose: one split, several equal splits, and
    a shorter last split where the planner allows one (the smallest shapes of a host search)."""
    M, S = dict(multi=True), dict(multi=True, short=True)
    return [
        _w("tile64-bf16", "bf16", 1, 1, 1, 8, 64, 1, 1, 0, T64),
        _w("tile64-m-bf16", "bf16", 5, 14, 14, 8, 64, 1, 1, 0, T64, **M),        # 2 x 8, a 20-pixel last step
        _w("tile64-s-bf16", "bf16", 64, 3, 7, 8, 64, 1, 1, 0, T64, **S),         # 21 steps: 11 + 10
        _w("tile64x128-bf16", "bf16", 1, 1, 1, 8, 128, 1, 1, 0, T64W),
        _w("tile64x128-m-bf16", "bf16", 5, 14, 14, 8, 128, 1, 1, 0, T64W, **M),
        _w("tile64x128-s-bf16", "bf16", 64, 3, 7, 8, 128, 1, 1, 0, T64W, **S),
        _w("tile128x64-bf16", "bf16", 1, 1, 1, 1024, 64, 7, 1, 3, T128),
        _w("tile128x64-s-bf16", "bf16", 59, 14, 14, 512, 64, 3, 1, 1, T128, **S),  # 181 steps: 13 x 13 + 12
        _w("tap3-bf16", "bf16", 16, 2, 2, 256, 2048, 3, 1, 1, TAP3),
        _w("tap3-m-bf16", "bf16", 7, 16, 16, 256, 512, 3, 1, 1, TAP3, **M),      # 4 x 7
        _w("tap3-s-bf16", "bf16", 124, 4, 4, 64, 2048, 3, 1, 1, TAP3, **S),      # 31 steps: 3 x 8 + 7
        _w("tap6-bf16", "bf16", 16, 2, 2, 64, 64, 3, 1, 1, TAP6),
        _w("tap6-m-bf16", "bf16", 128, 2, 2, 64, 64, 3, 1, 1, TAP6, **M),        # 2 x 4
        _w("tap6-s-bf16", "bf16", 59, 8, 8, 64, 64, 3, 1, 1, TAP6, **S),         # 59 steps: 11 x 5 + 4
        _w("tap3x128-bf16", "bf16", 16, 2, 2, 192, 5504, 3, 1, 1, TAP3W),
        _w("tap3x128-m-bf16", "bf16", 1024, 2, 2, 128, 4224, 3, 1, 1, TAP3W, **M),
        _w("tap3x128-s-bf16", "bf16", 260, 4, 4, 128, 4224, 3, 1, 1, TAP3W, **S),  # 65 steps: 33 + 32
        _w("gen6-bf16", "bf16", 7, 4, 4, 64, 64, 3, 1, 1, GEN6),
        _w("gen6-s-bf16", "bf16", 16, 7, 7, 64, 64, 3, 1, 1, GEN6, **S),         # 14 steps: 5 + 5 + 4
        _w("gen3-bf16", "bf16", 1, 4, 14, 256, 2048, 3, 1, 1, GEN3),
        _w("gen3-m-bf16", "bf16", 32, 7, 7, 256, 512, 3, 1, 1, GEN3, **M),       # 4 x 7
        _w("gen3-s-bf16", "bf16", 3, 28, 28, 64, 2048, 3, 1, 1, GEN3, **S),      # 42 steps: 3 x 11 + 9
        _w("gen3x128-bf16", "bf16", 14, 2, 2, 192, 5504, 3, 1, 1, GEN3W),
        _w("gen3x128-m-bf16", "bf16", 64, 4, 14, 128, 4224, 3, 1, 1, GEN3W, **M),
        _w("gen3x128-s-bf16", "bf16", 232, 7, 7, 64, 4224, 3, 1, 1, GEN3W, **S),  # 203 steps: 4 x 41 + 39
        _w("tile64-f32", "f32", 1, 1, 1, 8, 64, 1, 1, 0, T64),
        _w("tile64-m-f32", "f32", 4, 3, 3, 8, 64, 1, 1, 0, T64, **M),            # 2 x 1, a 4-pixel last step
        _w("tile64-s-f32", "f32", 7, 14, 14, 16, 128, 3, 1, 1, T64, **S),        # 43 steps: 21 x 2 + 1
        _w("tile128x64-f32", "f32", 1, 1, 1, 128, 512, 7, 1, 3, T128),
        _w("tile128x64-m-f32", "f32", 32, 3, 3, 256, 512, 3, 1, 1, T128, **M),   # 3 x 3
        _w("tile128x64-s-f32", "f32", 16, 5, 9, 128, 1024, 3, 1, 1, T128, **S),  # 23 steps: 8 + 8 + 7
        _w("tile64x128-f32", "f32", 1, 1, 1, 64, 1024, 7, 1, 3, T64W),
        _w("tile64x128-s-f32", "f32", 16, 5, 9, 64, 2048, 3, 1, 1, T64W, **S),
        _w("tap-f32", "f32", 8, 2, 2, 64, 64, 3, 1, 1, TAP3),
        _w("tap-m-f32", "f32", 16, 2, 2, 64, 64, 3, 1, 1, TAP3, **M),            # 2 x 1
        _w("tap-s-f32", "f32", 59, 4, 8, 64, 128, 3, 1, 1, TAP3, **S),           # 59 steps: 29 x 2 + 1
        _w("tapx128-f32", "f32", 8, 2, 2, 192, 5504, 3, 1, 1, TAP3W),
        _w("tapx128-m-f32", "f32", 28, 8, 8, 64, 2816, 3, 1, 1, TAP3W, **M),     # 7 x 8
        _w("tapx128-s-f32", "f32", 152, 2, 2, 64, 4224, 3, 1, 1, TAP3W, **S),    # 19 steps: 4 x 4 + 3
        _w("stem7-n1-f32", "f32", 1, 224, 224, 4, 64, 7, 2, 3, STEM, cin=3, **M),
        _w("stem7-n3-f32", "f32", 3, 224, 224, 4, 64, 7, 2, 3, STEM, cin=3, **M),
    ]


def edge_cases():
    M = dict(multi=True)
    return [
        # H != W, every family
        _w("hw5x9-bf16", "bf16", 3, 5, 9, 64, 64, 3, 1, 1, T64),
        _w("hw5x9-f32", "f32", 1, 5, 9, 64, 64, 3, 1, 1, T64, **M),
        _w("tap4x8-bf16", "bf16", 4, 4, 8, 64, 64, 3, 1, 1, TAP6),
        _w("tap8x2-bf16", "bf16", 8, 8, 2, 64, 64, 3, 1, 1, TAP6),
        _w("tap4x8-f32", "f32", 2, 4, 8, 64, 64, 3, 1, 1, TAP3, **M),
        _w("tap8x2-f32", "f32", 4, 8, 2, 64, 64, 3, 1, 1, TAP3, **M),
        _w("gen3x7-bf16", "bf16", 8, 3, 7, 64, 64, 3, 1, 1, GEN6),
        _w("gen4x14-bf16", "bf16", 2, 4, 14, 64, 64, 3, 1, 1, GEN6),
        _w("gen7x8-bf16", "bf16", 2, 7, 8, 64, 64, 3, 1, 1, GEN6),
        _w("gen7x2-bf16", "bf16", 8, 7, 2, 64, 64, 3, 1, 1, GEN6),
        # stride 2 on an odd image; 1x1 stride 2 (non-identity addressing); 1x1 stride 1 (ident)
        _w("s2odd-bf16", "bf16", 3, 7, 7, 64, 64, 3, 2, 1, T64),
        _w("s2odd-f32", "f32", 3, 7, 7, 64, 64, 3, 2, 1, T64, **M),
        _w("1x1s2-bf16", "bf16", 3, 7, 5, 64, 64, 1, 2, 0, T64),
        _w("1x1s2-f32", "f32", 3, 7, 5, 64, 64, 1, 2, 0, T64, **M),
        _w("ident-bf16", "bf16", 3, 7, 5, 64, 64, 1, 1, 0, T64),
        _w("ident-f32", "f32", 3, 7, 5, 64, 64, 1, 1, 0, T64, **M),
        # a 7x7 / s2 / p3 layer that is not the ImageNet stem: 49 taps, padded Kg, cin 3 < cp
        _w("k7-bf16", "bf16", 2, 16, 16, 8, 64, 7, 2, 3, T64, cin=3),
        _w("k7-f32", "f32", 2, 16, 16, 4, 64, 7, 2, 3, T64, cin=3, **M),
        # 3x3 with the smallest cp: Kg 72 -> 128 (fp32 cp 4: 36 -> 64), cin < cp
        _w("cp8-bf16", "bf16", 2, 5, 7, 8, 64, 3, 1, 1, T64, cin=5),
        _w("cp8-f32", "f32", 2, 5, 7, 8, 64, 3, 1, 1, T64, cin=5, **M),
        _w("cp4-f32", "f32", 2, 5, 7, 4, 64, 3, 1, 1, T64, cin=3, **M),
        _w("cp16-bf16", "bf16", 3, 5, 7, 16, 64, 3, 1, 1, T64),
        # fewer pixels than one step; one pixel more than a whole step
        _w("px9-bf16", "bf16", 1, 3, 3, 64, 64, 3, 1, 1, T64),
        _w("px9-f32", "f32", 1, 3, 3, 64, 64, 3, 1, 1, T64),
        _w("px65-bf16", "bf16", 1, 5, 13, 64, 64, 3, 1, 1, T64),
        _w("px33-f32", "f32", 1, 3, 11, 64, 64, 3, 1, 1, T64, **M),
    ]


def numerics_cases():
    M = dict(multi=True)
    return [
        _w("num-tile-bf16", "bf16", 5, 14, 14, 8, 64, 1, 1, 0, T64, **M),
        _w("num-tile3x3-bf16", "bf16", 3, 7, 7, 64, 64, 3, 2, 1, T64),
        _w("num-tap-bf16", "bf16", 128, 2, 2, 64, 64, 3, 1, 1, TAP6, **M),
        _w("num-gen-bf16", "bf16", 16, 7, 7, 64, 64, 3, 1, 1, GEN6, multi=True, short=True),
        _w("num-tile-f32", "f32", 3, 7, 7, 64, 64, 3, 2, 1, T64, **M),
        _w("num-tap-f32", "f32", 4, 8, 2, 64, 64, 3, 1, 1, TAP3, **M),
        _w("num-stem7-f32", "f32", 1, 224, 224, 4, 64, 7, 2, 3, STEM, cin=3, **M),
    ]


ROUTE_CASES, EDGE_CASES, NUMERICS = route_cases(), edge_cases(), numerics_cases()
ALL_EXACT = ROUTE_CASES + EDGE_CASES

# (kind, f32, br, bc, ns): the launch tables kW2Kernels, kW3Kernels, kW2fKernels, kW3fKernels + the stem's
COMPILED = {("tile", False, 128, 128, 4), ("tile", False, 128, 64, 3), ("tile", False, 64, 128, 3),
            ("tile", False, 64, 64, 3)} \
    | {(kind, False, 192, bc, ns) for kind in ("tap_reuse", "tap_reuse_general") for bc in (64, 128) for ns in (3, 6)} \
    | {("tile", True, br, bc, 3) for br in (64, 128) for bc in (64, 128)} \
    | {("tap_reuse", True, 192, 64, 3), ("tap_reuse", True, 192, 128, 3), ("stem7", True, 0, 0, 0)}
UNREACHED = {("tile", False, 128, 128, 4), ("tap_reuse", False, 192, 128, 6), ("tap_reuse_general", False, 192, 128, 6),
             ("tile", True, 128, 128, 3)}
REACHED = COMPILED - UNREACHED
NO_SHORT_LAST = {("stem7", True, 0, 0, 0)}  # reached, but no case with steps % kps != 0


# ---------------------------------------------------------------------------- the reduction alone
@dataclass(frozen=True)
class RCase:
    """Synthetic integer slabs [splits][oc][kg] for psx_wgrad_reduce alone."""
    id: str
    oc: int
    cin: int
    ic: int
    k: int
    splits: int

    @property
    def kg(self):
        return -(-(self.k * self.k * self.ic) // 64) * 64


@lru_cache(maxsize=None)
def reduce_slabs(rc):
    """Integers in [-4, 4], float64; NaN in the padded channels cin .. ic-1 and in the padding
    columns >= R S ic, which no reduction may let through."""
    gen = torch.Generator().manual_seed(rc.oc + 31 * rc.splits + rc.ic)
    RS = rc.k * rc.k
    s = torch.full((rc.splits, rc.oc, rc.kg), NAN, dtype=torch.float64)
    v = _ints(gen, (rc.splits, rc.oc, RS, rc.ic), 4)
    v[..., rc.cin:] = NAN
    s[:, :, :RS * rc.ic] = v.reshape(rc.splits, rc.oc, RS * rc.ic)
    return s


def _r(tag, oc, cin, ic, k, splits):
    return [RCase(f"{tag}-oc{oc}-c{cin}of{ic}-k{k}-s{s}", oc, cin, ic, k, s) for s in splits]


def reduce_cases():
    """wgrad_reduce2_kernel: items = R S CW / 4, G = min(splits, 256 / items) split groups."""
    out = []
    out += _r("g64", 64, 64, 64, 1, (1, 7, 8, 9, 513))      # CW 16: 4 items, G up to 64 (8 G + 1 = 513)
    out += _r("g16", 1024, 64, 64, 1, (1, 9, 16, 129))      # CW 64: 16 items, G up to 16
    out += _r("g7", 64, 64, 64, 3, (1, 7, 8, 9, 57))        # 3x3, CW 16: 36 items, G up to 7 (8 G + 1 = 57)
    out += _r("pass1", 1024, 64, 64, 3, (1, 9))             # 3x3, CW 64: 144 items, G 1, one pass
    out += _r("pass2", 1024, 64, 64, 5, (1, 9))             # 5x5, CW 64: 400 items, G 1, two passes
    out += _r("k7", 64, 16, 16, 7, (1, 8, 9))               # 7x7, IC 16: 196 items
    for oc in (1024, 960, 512, 448):                        # IC 64: CW 64 | 32 | 32 | 16 (the 1024-workgroup rule)
        out += _r("cw", oc, 64, 64, 1, (3,))
    out += _r("cw32", 512, 64, 64, 3, (9,))                 # CW 32: 72 items, G 3
    out += _r("cin", 64, 40, 64, 3, (1, 9))                 # CW 16: chunk 2 half valid, chunk 3 padded (cv <= 0)
    out += _r("cin", 1024, 40, 64, 1, (3,))                 # CW 64: one chunk, 40 of 64 valid
    out += _r("ic96", 1024, 96, 96, 1, (1, 9))              # CW must divide IC (64 does not)
    out += _r("ic80", 512, 80, 80, 3, (3,))                 # (32 does not)
    out += _r("ic192", 1024, 192, 192, 1, (3,))             # the control: three chunks of 64
    out += _r("ic48", 64, 48, 48, 3, (3,))
    # wgrad_reduce_kernel (one thread per column): IC 4 and 8, R S > 49; the pre-sum of the layers
    # with fewer than 128 workgroups from 33 splits on; 128 workgroups: no pre-sum
    out += _r("v1", 64, 3, 4, 7, (1, 8, 31, 32, 33, 47, 48, 49, 256))
    out += _r("v1", 64, 5, 8, 3, (5, 33, 65))
    out += _r("v1", 64, 16, 16, 9, (3, 33, 70))             # 81 taps, 336 workgroups
    out += _r("v1", 128, 3, 4, 7, (33, 70))                 # 128 workgroups: the 32-slab main loop, no pre-sum
    return out


REDUCE_CASES = reduce_cases()
# the layers of each batched launch: (id, oc, cin, ic, k, splits)
BATCHES = [[("b0", 64, 64, 64, 3, 9)],
           [("b0", 64, 64, 64, 3, 9), ("b1", 128, 40, 64, 1, 57)],
           [("b0", 1024, 64, 64, 1, 3), ("b1", 64, 16, 16, 7, 8), ("b2", 64, 96, 96, 3, 2)],
           [("b0", 64, 64, 64, 3, 9), ("b1", 1024, 96, 96, 1, 3), ("b2", 512, 64, 64, 3, 1), ("b3", 64, 16, 16, 5, 17)]]
BATCHES = [[RCase(*t) for t in b] for b in BATCHES]


# ---------------------------------------------------------------------------- wrong variants
# name -> the cases on which the deliberately wrong reference must differ from the true one
WRONG_WGRAD = {
    "split_off_by_one": ["tile64-m-bf16", "tap-m-f32", "gen6-s-bf16"],
    "last_step_dropped": ["tile64-m-bf16", "tile64-m-f32", "px65-bf16"],
    "rs_swapped": ["hw5x9-bf16", "k7-f32"],
    "hw_swapped": ["hw5x9-bf16", "tap4x8-f32", "gen3x7-bf16"],
    "pad_ignored": ["px9-f32", "k7-bf16"],
    "stride_ignored": ["s2odd-bf16", "1x1s2-f32"],
    "chanpad_kept": ["k7-bf16", "cp4-f32"],
    "tap_c_transposed": ["cp8-bf16", "tap-f32"],
}
WRONG_REDUCE = {
    "presum_slab_stride": ["v1-oc64-c3of4-k7-s33", "v1-oc64-c3of4-k7-s256"],
    "chanpad_kept": ["cin-oc64-c40of64-k3-s9"],
}


# ---------------------------------------------------------------------------- CPU tests
def test_references_match_a_naive_loop_nest_and_torch():
    """ref_slabs summed over the splits, through reduce_reference, equals a naive loop nest on tiny
    shapes and torch.nn.grad.conv2d_weight in float64 (exact operands: equality)."""
    for k, stride, pad, hw in ((3, 1, 1, (4, 3)), (3, 2, 1, (5, 4)), (1, 2, 0, (3, 4)), (7, 2, 3, (6, 5)), (1, 1, 0,
                                                                                                             (2, 3))):
        c = WCase(id=f"tiny{k}{stride}", f32=True, n=2, h=hw[0], w=hw[1], cp=4, oc=3, k=k, stride=stride, pad=pad, cin=3)
        sp = -(-c.npix // 8)  # splits of two 4-pixel steps, the last one shorter or partial
        path = dict(kind="tile", splits=sp, kps=2, pix=4)
        x, dy, _, _ = operands(c)
        want = naive_wgrad(x, dy, k, stride, pad)
        assert torch.equal(ref_oihw(c, path).double(), want)
        assert torch.equal(torch_wgrad(c), want)
        slabs = ref_slabs(c, path)
        assert not slabs[:, :, k * k * 4:].any() and slabs.shape == (sp, 3, c.kg)
        assert not slabs[:, :, :k * k * 4].reshape(sp, 3, k * k, 4)[..., 3].any()  # the padded channel


@pytest.mark.parametrize("case", ALL_EXACT, ids=ids(ALL_EXACT))
def test_exact_cases_take_their_route_and_match_torch(case):
    """The planner takes the route the case names; the slabs are exact integers below 2^24 with
    zero padding columns; their reduction equals torch's float64 weight gradient."""
    path = query_route(case)
    slabs = ref_slabs(case, path)
    assert slabs.shape[0] == path["splits"]
    assert float(ref_slabs(case, path, absolute=True).sum(0).max()) < LIM
    assert not slabs[:, :, case.k ** 2 * case.cp:].any()
    assert torch.equal(slabs, slabs.round())
    got = ref_oihw(case, path)
    assert torch.equal(got.double(), torch_wgrad(case)), case.id
    if case.multi and path["kind"] != "stem7":
        assert all(bool(s.any()) for s in slabs), (case.id, "an empty split")


def test_case_ids_are_unique():
    names = ids(ALL_EXACT + NUMERICS) + ids(REDUCE_CASES)
    assert len(names) == len(set(names))


def test_reached_instantiations():
    """The case table reaches exactly REACHED, and REACHED with UNREACHED is every compiled
    instantiation. Each reached one has a case with one split, one with several, and one whose last
    split is shorter than the others, unless it is listed in NO_SHORT_LAST (the stem, whose split
    scheme is its own; the planner gives every other reached instantiation a shorter last split)."""
    assert {c.inst for c in ROUTE_CASES} == REACHED
    assert REACHED | UNREACHED == COMPILED and not REACHED & UNREACHED and len(COMPILED) == 19
    assert NO_SHORT_LAST <= REACHED
    for inst in REACHED - {("stem7", True, 0, 0, 0)}:
        assert {c.multi for c in ROUTE_CASES if c.inst == inst} == {False, True}, inst
    for inst in REACHED:
        assert any(c.short for c in ROUTE_CASES if c.inst == inst) == (inst not in NO_SHORT_LAST), inst


def test_unreached_instantiations_stay_unreached():
    """No geometry of this search takes an instantiation outside REACHED: k 1 / 3 / 7, images 1 to
    112 (some not square), cp 4 to 2048, oc 64 to 8192, n 1 to 1024. A planner change that starts
    choosing one of UNREACHED needs a case in route_cases first."""
    from psx.ops import kernels as K
    seen = set()
    hws = [(a, a) for a in (1, 2, 4, 7, 8, 14, 16, 28, 32, 56, 64, 112)] + [(4, 8), (4, 14), (5, 9)]
    for f32 in (False, True):
        for k, pad in ((1, 0), (3, 1), (7, 3)):
            for stride in (1, 2):
                for h, w in hws:
                    for cp in (4, 8, 64, 128, 192, 512, 2048):
                        if cp < 8 and not f32:
                            continue
                        kg = -(-(k * k * cp) // 64) * 64
                        for oc in (64, 128, 512, 2048, 5504, 8192):
                            for n in (1, 3, 8, 16, 59, 128, 1024):
                                p = K.conv_wgrad2_path(n, h, w, cp, oc, k, stride, pad, kg, f32)
                                if isinstance(p, dict):
                                    seen.add((p["kind"], p["f32"], p["br"], p["bc"], p["ns"]))
    assert seen <= REACHED, seen - REACHED
    assert seen >= REACHED - {("stem7", True, 0, 0, 0)}, REACHED - seen


@pytest.mark.parametrize("name", list(WRONG_WGRAD), ids=list(WRONG_WGRAD))
def test_wrong_variants_are_caught(name):
    """Each deliberately wrong weight gradient differs from the true reference on every case named
    for it: in a slab where the mistake is in the GEMM or its splits (the boundary mistakes leave
    the sum over the splits unchanged: only the per-slab comparison sees them), in the reduced
    gradient where it is in the permutation."""
    table = {c.id: c for c in ALL_EXACT}
    for cid in WRONG_WGRAD[name]:
        case = table[cid]
        path = query_route(case)
        if name in BUGS_REDUCE:
            assert not torch.equal(ref_oihw(case, path, bug=name), ref_oihw(case, path)), (name, cid)
        else:
            assert not torch.equal(ref_slabs(case, path, bug=name), ref_slabs(case, path)), (name, cid)
    if name == "split_off_by_one":
        c = table["tap-m-f32"]
        p = query_route(c)
        assert torch.equal(ref_oihw(c, p, bug=name), ref_oihw(c, p))  # two boundary errors cancel in the sum


@pytest.mark.parametrize("name", list(WRONG_REDUCE), ids=list(WRONG_REDUCE))
def test_wrong_reductions_are_caught(name):
    table = {c.id: c for c in REDUCE_CASES}
    for cid in WRONG_REDUCE[name]:
        rc = table[cid]
        s = reduce_slabs(rc)
        good = reduce_reference(s, rc.cin, rc.ic, rc.k, 1.0, False)
        bad = reduce_reference(s, rc.cin, rc.ic, rc.k, 1.0, False, bug=name)
        assert not bool(torch.isnan(good).any())
        assert not torch.equal(good, bad.nan_to_num(nan=1e30)), (name, cid)


def test_reduce_cases_are_exact():
    """The synthetic slabs' sums are integers exact in fp32, NaN exactly where the reduction must
    not look, and the pre-sum cases sit where presum_applies says."""
    for rc in REDUCE_CASES:
        s = reduce_slabs(rc)
        ref = reduce_reference(s, rc.cin, rc.ic, rc.k, 1.0, False)
        assert ref.shape == (rc.oc, rc.cin, rc.k, rc.k) and not bool(torch.isnan(ref).any())
        assert 4 * rc.splits < LIM and rc.kg % 64 == 0
    pre = {c.id for c in REDUCE_CASES if presum_applies(c.splits, c.oc, c.kg, c.ic, c.k)}
    assert pre == {f"v1-oc64-c3of4-k7-s{s}" for s in (33, 47, 48, 49, 256)} | {"v1-oc64-c5of8-k3-s33",
                                                                                "v1-oc64-c5of8-k3-s65"}


@pytest.mark.parametrize("case", NUMERICS, ids=ids(NUMERICS))
def test_torch_fp32_lies_inside_the_numerics_bound(case):
    path = query_route(case)
    y = torch_wgrad(case, numerics=True, dtype=F32)
    for scale in SCALES:
        for fp16 in (False, True):
            ref, bound = numerics_reference(case, path, scale, fp16)
            got = (y * scale).to(F16) if fp16 else y * scale
            assert bool(within(got, ref, bound).all()), (case.id, scale, fp16)
            assert bool((bound > 0).any())


def test_refusals():
    """route_wgrad's refusals through the query: OC % 64, Kg % 64, and an input channel count that
    is no power of two (or below one 16-byte chunk) on the tile routes of either dtype, whose
    column decode tap = column >> log2(IC) needs one. The tap-reuse routes take any IC % 64 == 0."""
    from psx.ops import kernels as K
    assert K.conv_wgrad2_path(8, 16, 16, 64, 96, 3, 1, 1, 576, False) == -2
    assert K.conv_wgrad2_path(8, 16, 16, 64, 64, 3, 1, 1, 600, False) == -2
    for f32 in (False, True):
        assert K.conv_wgrad2_path(8, 16, 16, 48, 64, 3, 1, 1, 448, f32) == -2
        assert K.conv_wgrad2_path(8, 16, 16, 48, 64, 1, 1, 0, 64, f32) == -2
        assert K.conv_wgrad2_path(8, 16, 16, 24, 64, 7, 2, 3, 1216, f32) == -2
        assert K.conv_wgrad2_path(8, 16, 16, 192, 64, 3, 2, 1, 1728, f32) == -2
        assert K.conv_wgrad2_path(8, 16, 16, 192, 64, 3, 1, 1, 1728, f32)["kind"] == "tap_reuse"
    assert K.conv_wgrad2_path(8, 16, 16, 4, 64, 3, 1, 1, 64, False) == -2          # bf16: IC % 8
    assert K.conv_wgrad2_path(8, 14, 14, 192, 64, 3, 1, 1, 1728, False)["kind"] == "tap_reuse_general"
    assert K.conv_wgrad2_path(8, 14, 14, 192, 64, 3, 1, 1, 1728, True) == -2       # fp32: no general-width kernel
