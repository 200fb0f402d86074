"""The BatchNorm kernels of csrc/kernels/bn.hip and csrc/kernels/bnfin.hpp, directly, against the
fp64 references and the bounds of tests/test_bn_cpu.py, on every dispatch path: every template
instantiation, deterministic mode off and on, and the geometry branches. Every buffer a kernel sees
lies inside a larger allocation of canaries; outputs are pre-filled with NaN, so an element that is
not written fails; every element is held to its bound. The consumers of slot sums are fed
host-built slots (float rows, or fixed-point pairs from the host encoder) and never a producer's.

Which test reaches which branch:

  psx_bn_finalize            test_bn_finalize[float / det]: sshift none (plain, big) and given
    bn_finalize_kernel       (big_shift: mean 100 / std 1), running statistics and sshift_next none
                             and given; C in 8, 40, 64 (partial 32-channel block, second block); T in
                             1, 8, 19 (second trip of the 8-way slot loop); count 1; the constant
                             channels 3 and 4 (variance 0 / clamped, invstd = 1 / sqrt(eps))
  psx_bn_eval_affine         test_bn_eval_affine: C in 8, 300
  psx_bn_apply               test_bn_apply[dtype-mode-relu]: all 12 instantiations; C in 8, 48, 64 at
    bn_apply_kernel<T,M,R>   npix 33; second grid-stride trip: C 64, npix 65,537
  psx_bn_apply_fin           test_bn_apply_fin[dtype-mode-relu-float / det]: the same 12 x det
    bn_apply_fin_kernel      fixed hoist: C 8, 64 at npix 33; second trip C 64, npix 16,385 (grid cap
    bn_fin_lds               512); not-fixed: C 48 at npix 33 and 21,847 (the channel group changes
    slot_reduce2             between trips); slot_reduce2: C in 8, 256, 512, 1024, 1536, 2048 at npix
                             64 (G = 8, 4, 2, 1, mixed 1 -> 2, two passes; C 2048: 69,632 B of LDS);
                             side outputs from workgroup 0 only and used by all: the output is held
                             to the reference of the affine that was written; running statistics
                             and sshift_next moved once; equal to bn_finalize + bn_apply
  psx_bn_bwd_reduce          test_bn_bwd_reduce[dtype-mask-two-float / det-fin]: all 8 instantiations
    bn_bwd_reduce_kernel     x det x in-launch finalize (fin1, fin2, zeroed counter); C in 8, 64, 2048
    stat_add                 (tpp 256, 32, 1); npix in 1, 64, 65, 577 (one pixel in the last
    bn_bwd_finalize_block    workgroup; 10 workgroups over 8 slot rows); C 8 at npix 32,833 (ppb 65);
                             every slot row held to its own bound; det: two launches give identical
                             words, decoded inside the tighter bound; test_bn_bwd_reduce_rejects_c48
    fix_add                  test_fix_add_matches_the_host_encoder: the slot words of known partials
                             equal the host encoder's, poison included
  psx_bn_bwd_finalize        test_bn_bwd_finalize[sink-float / det-NS-which]: fp32 / fp16 sink, NS 2 /
    bn_bwd_finalize_kernel   3, which 1 / 2, gscale 1 and 1/3; C in 8, 40, 64; T in 1, 8, 19
  psx_bn_bwd_apply           test_bn_bwd_apply[dtype-mask-two-dzout]: all 16; shapes as bn_apply;
    bn_bwd_apply_kernel      dzout bit for bit
  psx_bn_bwd_apply_fin       test_bn_bwd_apply_fin[dtype-mask-two-dzout-float / det]: the same 16 x
    bn_bwd_apply_fin_kernel  det; shapes as bn_apply_fin (C 2048: 86,016 B of LDS); coefficients,
    bn_bwd_fin_lds           dgamma, dbeta from workgroup 0 and used by all
  non-finite g               test_nonfinite_gradient_reaches_dgamma[float / det]: NaN / Inf in g make
                             dgamma / dbeta NaN (poisoned entries in det mode), other channels intact
  the default path, chained  test_block_output_chain[dtype-mean0 / mean100-float / det]: bn_apply_fin
                             (mode 2, ReLU) -> bn_bwd_reduce (NS 3) -> bn_bwd_apply_fin (which 1, 2)
                             against torch float64 autograd of F.batch_norm, C 64, npix 577

The worst error / bound ratio of every kernel is printed when the module ends (profiles/
bn_paths.txt holds a run's figures)."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from psx.ops import kernels as K

from .test_bn_cpu import (APPLY_SHAPES, BF16, CHAIN, EPS, F32, MOMENTUM, REDUCE_SHAPES, SLOTS, STATS_C, STATS_T, U,
                          bn_apply_reference, bn_bwd_apply_reference, bn_bwd_coef_reference, bn_bwd_sums_reference,
                          bn_eval_affine_reference, bn_inputs, bn_params, bn_stats_reference, det_buffer, det_slots,
                          ew_grid, float_slots, reduce_geometry, slot_total, stats_case, stats_slots, true_saved)
from .test_lars_cpu import f32
from .test_sgd_cpu import assert_within
from .test_sgd_gpu import Placed, assert_same_bits, bits

pytestmark = pytest.mark.gpu

F16 = torch.float16
NAN = float("nan")
RATIOS = {}   # (kernel, dtype / mode) -> worst error / bound
FIGURES = {}  # other measured figures
DT = pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
DET = pytest.mark.parametrize("det", [False, True], ids=["float", "det"])
FIN_SHAPES = APPLY_SHAPES + ((64, 16385), (48, 21847)) + tuple((C, 64) for C in (8, 256, 512, 1024, 1536, 2048))
NPART = 19  # host partials per slot buffer: two or three adds per slot row


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(RATIOS):
        print("bn_paths ratio", *key, "%.4f" % RATIOS[key])
    for key in sorted(FIGURES):
        print("bn_paths figure", key, FIGURES[key])


def held(x, ref, bound, key, what):
    """Every element of x within its bound of ref; the worst ratio is recorded first."""
    x = x.detach().cpu().double().reshape(ref.shape)
    r = ((x - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(r.max()))
    assert_within(x, ref, bound, (key,) + tuple(what))


class Bufs:
    """The placed buffers of one launch: inputs (checked unchanged) and NaN-filled outputs."""

    def __init__(self):
        self.ins, self.outs = [], []

    def put(self, x, fill=None, inout=False):
        p = Placed(x.contiguous().view(-1), 0, fill)
        (self.outs if inout else self.ins).append(p)
        return p

    def out(self, n, dtype=F32):
        return self.put(torch.full((n,), NAN, dtype=dtype), inout=True)

    def check(self, what):
        torch.cuda.synchronize()
        assert all(p.intact() for p in self.ins + self.outs), ("canaries",) + tuple(what)
        assert all(p.unchanged() for p in self.ins), ("an input was written",) + tuple(what)


def slot_buffer(partials, det, nrows=SLOTS):
    """Host-built slots for a consumer: (what the reference reads, the fp32 buffer for the kernel)."""
    if det:
        pairs = det_slots(partials, nrows)
        return pairs, det_buffer(pairs)
    rows = float_slots(partials, nrows)
    return rows, rows.reshape(-1)


@contextlib.contextmanager
def det_mode(on):
    """Deterministic mode for the launches inside, off again whatever happens."""
    try:
        K.set_deterministic(on)
        yield
    finally:
        K.set_deterministic(False)


def dname(dtype):
    return {F32: "fp32", BF16: "bf16", F16: "fp16"}[dtype]


# ---------------------------------------------------------------------------- forward finalize
@DET
def test_bn_finalize(det):
    with det_mode(det):
        for C in STATS_C:
            P = bn_params(C)
            for T in STATS_T:
                for kind in ("plain", "big", "big_shift") + (("count1",) if T == 1 else ()):
                    slots, n, k = stats_case(C, T, kind)
                    for full in (False, True):  # running statistics and sshift_next given or not
                        B = Bufs()
                        src, buf = slot_buffer(slots, det, T)
                        part = B.put(buf)
                        gamma, beta = B.put(P["gamma"]), B.put(P["beta"])
                        sshift = B.put(k) if k is not None else None
                        aff, sav = B.out(2 * C), B.out(2 * C)
                        rm = B.put(P["run_mean"], inout=True) if full else None
                        rv = B.put(P["run_var"], inout=True) if full else None
                        nxt = B.out(C) if full else None
                        K.bn_finalize(part.view, T, C, n, gamma.view, beta.view, EPS, MOMENTUM,
                                      rm.view if full else None, rv.view if full else None, aff.view, sav.view,
                                      sshift=sshift.view if sshift else None, sshift_next=nxt.view if full else None)
                        what = (C, T, kind, full, det)
                        B.check(what)
                        ref, bound = bn_stats_reference(src, n, k, P["gamma"], P["beta"], EPS, MOMENTUM,
                                                        P["run_mean"] if full else None, P["run_var"] if full else None,
                                                        det=det, fp32_depth=0 if det else -(-T // 8))
                        key = ("bn_finalize", "det" if det else "float")
                        got = dict(scale=aff.view[:C], shift=aff.view[C:], mean=sav.view[:C], invstd=sav.view[C:])
                        if full:
                            got.update(run_mean=rm.view, run_var=rv.view, sshift_next=nxt.view)
                            assert_same_bits(nxt.view, sav.view[:C], what)
                        for name, x in got.items():
                            held(x, ref[name], bound[name], key, (name,) + what)
                    if kind != "big_shift":
                        assert float(sav.view[C + 3]) == f32(1.0 / math.sqrt(f32(EPS))), what


def test_bn_eval_affine():
    """rsqrtf's allowance: no accuracy table of the HIP math library is at hand, so twice the
    worst relative deviation of torch's own fp32 rsqrt (on the device, same inputs) from fp64."""
    for C in (8, 300):
        P = bn_params(C)
        x = (P["run_var"] + torch.tensor(f32(EPS), dtype=F32))
        dev = torch.rsqrt(x.cuda()).cpu().double()
        exact = 1.0 / torch.sqrt(x.double())
        r = 2 * float(((dev - exact).abs() / exact).max())
        FIGURES["rsqrtf allowance (2 x torch fp32 rsqrt vs fp64, relative), C %d" % C] = "%.3e" % r
        B = Bufs()
        ins = [B.put(P[n]) for n in ("gamma", "beta", "run_mean", "run_var")]
        aff = B.out(2 * C)
        K.bn_eval_affine(C, *(p.view for p in ins), EPS, aff.view)
        B.check((C,))
        sc, sh, bsc, bsh = bn_eval_affine_reference(P["gamma"], P["beta"], P["run_mean"], P["run_var"], EPS, r)
        held(aff.view[:C], sc, bsc, ("bn_eval_affine", "fp32"), ("scale", C))
        held(aff.view[C:], sh, bsh, ("bn_eval_affine", "fp32"), ("shift", C))


# ---------------------------------------------------------------------------- forward apply
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@DT
def test_bn_apply(dtype, mode, relu):
    for C, npix in APPLY_SHAPES + ((64, 65537),):
        x, P = bn_inputs(C, npix, dtype), bn_params(C)
        assert npix < 65537 or (npix * C // 8 > 2048 * 256 and ew_grid(npix * C // 8) == 2048)
        B = Bufs()
        y, res = B.put(x["y1"]), (B.put(x["y2"]) if mode else None)
        a1 = B.put(torch.cat([P["gamma"], P["beta"]]))
        a2 = B.put(torch.cat([P["gamma2"], P["beta2"]])) if mode == 2 else None
        out = B.out(npix * C, dtype)
        K.bn_apply(y.view, a1.view, out.view, C, relu=relu, res=res.view if mode else None,
                   affine2=a2.view if mode == 2 else None)
        B.check((C, npix))
        ref, bound = bn_apply_reference(x["y1"], P["gamma"], P["beta"], x["y2"], P["gamma2"], P["beta2"], relu, mode)
        held(out.view, ref, bound, ("bn_apply", dname(dtype)), (C, npix, mode, relu))


def _fwd_slots(y, det, k):
    return slot_buffer(stats_slots(y, SLOTS, k, nparts=NPART), det)


def _stats_held(key, C, aff, sav, ref, bound, what, extra=()):
    got = dict(scale=aff.view[:C], shift=aff.view[C:], mean=sav.view[:C], invstd=sav.view[C:])
    got.update(extra)
    for name, x in got.items():
        held(x, ref[name], bound[name], key, (name,) + tuple(what))


@DET
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@DT
def test_bn_apply_fin(dtype, mode, relu, det):
    """BN 1: shifted sums (sshift given), running statistics and sshift_next written; the shortcut
    BN of mode 2: unshifted, no running statistics."""
    key = ("bn_apply_fin", dname(dtype) + (" det" if det else ""))
    with det_mode(det):
        for C, npix in FIN_SHAPES:
            x, P = bn_inputs(C, npix, dtype), bn_params(C)
            what = (C, npix, mode, relu, det)
            k1 = (x["y1"].double().mean(0) + 0.01).float()
            B = Bufs()
            src1, buf1 = _fwd_slots(x["y1"], det, k1)
            part1, sshift = B.put(buf1), B.put(k1)
            y, res = B.put(x["y1"]), (B.put(x["y2"]) if mode else None)
            g1, b1 = B.put(P["gamma"]), B.put(P["beta"])
            rm, rv = B.put(P["run_mean"], inout=True), B.put(P["run_var"], inout=True)
            aff1, sav1, nxt = B.out(2 * C), B.out(2 * C), B.out(C)
            fin1 = K.bn_fin(g1.view, b1.view, rm.view, rv.view, aff1.view, sav1.view, None, npix, EPS, MOMENTUM, C,
                            sshift=sshift.view, sshift_next=nxt.view)
            part2 = fin2 = None
            if mode == 2:
                src2, buf2 = _fwd_slots(x["y2"], det, None)
                part2, g2, b2 = B.put(buf2), B.put(P["gamma2"]), B.put(P["beta2"])
                aff2, sav2 = B.out(2 * C), B.out(2 * C)
                fin2 = K.bn_fin(g2.view, b2.view, None, None, aff2.view, sav2.view, None, npix, EPS, MOMENTUM, C)
            out = B.out(npix * C, dtype)
            K.bn_apply_fin(y.view, part1.view, fin1, out.view, C, relu=relu, res=res.view if mode else None,
                           part2=part2.view if part2 else None, fin2=fin2)
            B.check(what)
            ref1, bd1 = bn_stats_reference(src1, npix, k1, P["gamma"], P["beta"], EPS, MOMENTUM, P["run_mean"],
                                           P["run_var"], det=det)
            # one momentum update: a second one would be outside (the workgroups are many at the
            # large shapes; only workgroup 0 writes)
            _stats_held(key, C, aff1, sav1, ref1, bd1, what,
                        dict(run_mean=rm.view, run_var=rv.view, sshift_next=nxt.view))
            twice = (1 - f32(MOMENTUM)) * ref1["run_mean"] + f32(MOMENTUM) * ref1["mean"]
            assert bool(((twice - ref1["run_mean"]).abs() > bd1["run_mean"]).any())
            sc2 = sh2 = None
            if mode == 2:
                ref2, bd2 = bn_stats_reference(src2, npix, None, P["gamma2"], P["beta2"], EPS, MOMENTUM, None, None,
                                               det=det)
                _stats_held(key, C, aff2, sav2, ref2, bd2, what)
                sc2, sh2 = aff2.view[:C].cpu(), aff2.view[C:].cpu()
            # the output against the affine that workgroup 0 wrote: every workgroup used the same
            sc, sh = aff1.view[:C].cpu(), aff1.view[C:].cpu()
            ref, bound = bn_apply_reference(x["y1"], sc, sh, x["y2"], sc2, sh2, relu, mode)
            held(out.view, ref, bound, key, ("out",) + what)
            if (C, npix) == (64, 33):  # the same slots through bn_finalize + bn_apply
                S = Bufs()
                a1, s1 = S.out(2 * C), S.out(2 * C)
                K.bn_finalize(part1.view, SLOTS, C, npix, g1.view, b1.view, EPS, MOMENTUM, None, None, a1.view,
                              s1.view, sshift=sshift.view)
                a2 = None
                if mode == 2:
                    a2, s2 = S.out(2 * C), S.out(2 * C)
                    K.bn_finalize(part2.view, SLOTS, C, npix, g2.view, b2.view, EPS, MOMENTUM, None, None, a2.view,
                                  s2.view)
                sep = S.out(npix * C, dtype)
                K.bn_apply(y.view, a1.view, sep.view, C, relu=relu, res=res.view if mode else None,
                           affine2=a2.view if a2 else None)
                S.check(what)
                # both lie within `bound` of references whose affines differ by at most the
                # finalize bounds
                slack = x["y1"].double().abs() * 2 * bd1["scale"] + 2 * bd1["shift"]
                if mode == 2:
                    slack = slack + x["y2"].double().abs() * 2 * bd2["scale"] + 2 * bd2["shift"]
                assert_within(out.view.cpu().view(npix, C), sep.view.cpu().double().view(npix, C), 2 * bound + slack,
                              ("fin vs separate",) + what)


# ---------------------------------------------------------------------------- backward reduce
def _coef_held(key, C, coef, dg, db, cref, cb, what):
    got = dict(k1=coef.view[:C], k2=coef.view[C:2 * C], k3=coef.view[2 * C:], dgamma=dg.view, dbeta=db.view)
    for name, x in got.items():
        held(x.float(), cref[name], cb[name], key, (name,) + tuple(what))


@pytest.mark.parametrize("fin", [False, True], ids=["sums", "fin"])
@DET
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@DT
def test_bn_bwd_reduce(dtype, mask, two, det, fin):
    key = ("bn_bwd_reduce", dname(dtype) + (" det" if det else ""))
    NS = 3 if two else 2
    scale = K.det_slot_scale() if det else 1
    with det_mode(det):
        for C, npix in REDUCE_SHAPES:
            x, P = bn_inputs(C, npix, dtype), bn_params(C)
            s1, s2 = true_saved(x["y1"]), true_saved(x["y2"])
            geo = reduce_geometry(npix, C)
            what = (C, npix, mask, two, det, fin)
            words = []
            for launch in range(2 if det else 1):
                B = Bufs()
                g, o, y1, y2 = B.put(x["g"]), B.put(x["o"]), B.put(x["y1"]), B.put(x["y2"])
                sv1, sv2 = B.put(s1), B.put(s2)
                part = B.put(torch.zeros(SLOTS * NS * C * scale), inout=True)
                f1 = f2 = None
                if fin:
                    cnt = B.put(torch.zeros(1, dtype=torch.int32), fill=-1, inout=True)
                    gm1, gm2 = B.put(P["gamma"]), B.put(P["gamma2"])
                    c1, dg1, db1 = B.out(3 * C), B.out(C), B.out(C)
                    c2, dg2, db2 = B.out(3 * C), B.out(C), B.out(C)
                    f1 = K.bn_bwd_fin(gm1.view, sv1.view, c1.view, dg1.view.data_ptr(), db1.view.data_ptr(),
                                      cnt.view.data_ptr(), npix, 1 / 3, C, False)
                    f2 = K.bn_bwd_fin(gm2.view, sv2.view, c2.view, dg2.view.data_ptr(), db2.view.data_ptr(),
                                      cnt.view.data_ptr(), npix, 1 / 3, C, False) if two else None
                K.bn_bwd_reduce(g.view, o.view if mask else None, y1.view, sv1.view, part.view, npix, C,
                                y2=y2.view if two else None, saved2=sv2.view if two else None, fin1=f1, fin2=f2)
                B.check(what)
                words.append(bits(part.view).cpu().clone())
            if det:
                assert torch.equal(words[0], words[1]), ("two launches, different words",) + what
                rows = K.det_slot_values(part.view.cpu(), (SLOTS, NS, C))
            else:
                rows = part.view.cpu().double().view(SLOTS, NS, C)
            ref, bound = bn_bwd_sums_reference(x["g"], x["o"], x["y1"], s1, x["y2"] if two else None, s2, mask, geo,
                                               det)
            held(rows, ref, bound, key, ("rows",) + what)
            if fin:
                assert int(cnt.view[0]) == geo["wgs"], what
                tot, btot = ref.sum(0), bound.sum(0)
                for which, (gm, sv, c, dg, db) in enumerate(((P["gamma"], s1, c1, dg1, db1),
                                                             (P["gamma2"], s2, c2, dg2, db2))[:NS - 1], 1):
                    cref, cb = bn_bwd_coef_reference(tot[0], tot[which], npix, gm, sv, 1 / 3, btot[0], btot[which])
                    _coef_held(("bn_bwd_reduce fin", key[1]), C, c, dg, db, cref, cb, (which,) + what)


def test_fix_add_matches_the_host_encoder():
    """One pixel, no mask: the workgroup partial of sum dz is g itself, so the slot words are
    fix_add's of known fp32 values and must equal the host encoder's bit for bit: negative
    values, at and below 2^-41, just under 2^38, and 2^38 / Inf / NaN, which poison."""
    C = 64
    vals = [1.0, -1.0, 0.1, -0.1, 2.0 ** -41, -(2.0 ** -41), 2.0 ** -42 * 1.0000001, -(2.0 ** -42) * 1.0000001,
            3e-20, -3e-20, 1.4e-45, -1.4e-45, 2.0 ** 38 - 2.0 ** 14, -(2.0 ** 38 - 2.0 ** 14), 2.0 ** 38,
            -(2.0 ** 38), float("inf"), float("-inf"), NAN, 1234.5678, -2.25e4, 0.0]
    g = torch.tensor((vals * 3)[:C], dtype=F32).view(1, C)
    saved = torch.stack([torch.zeros(C), torch.ones(C)])
    with det_mode(True):
        B = Bufs()
        gd, y1, sv = B.put(g), B.put(torch.zeros(1, C)), B.put(saved)
        part = B.put(torch.zeros(SLOTS * 2 * C * K.det_slot_scale()), inout=True)
        K.bn_bwd_reduce(gd.view, None, y1.view, sv.view, part.view, 1, C)
        B.check(())
    words = part.view.cpu().view(torch.int64).view(SLOTS, 2, C, 2)
    want = det_slots(g)  # [SLOTS, C, 2]: the one partial in row 0
    assert torch.equal(words[:, 0], want), (words[0, 0], want[0])
    assert int((want[0, :, 1] < 0).sum()) == sum(1 for v in (vals * 3)[:C] if not abs(v) < 2.0 ** 38)


def test_bn_bwd_reduce_rejects_c48():
    z = torch.zeros(64 * 48, device="cuda")
    with pytest.raises(RuntimeError):
        K.bn_bwd_reduce(z, None, z, torch.ones(2 * 48, device="cuda"), torch.zeros(SLOTS * 2 * 48, device="cuda"),
                        64, 48)
    with pytest.raises(ValueError):
        reduce_geometry(64, 48)


# ---------------------------------------------------------------------------- backward finalize
def _bwd_partials(C, NS, n, seed=0):
    """Host partials [n, NS, C] of backward sums: mixed signs, magnitudes from 1e-3 to 30."""
    gen = torch.Generator().manual_seed(31 + C + 7 * NS + seed)
    return torch.randn(n, NS, C, generator=gen) * torch.logspace(-3, 1.5, C).view(1, 1, C)


def _param_saved(P, tag=""):
    return torch.stack([P["run_mean" + tag], 1.0 / torch.sqrt(P["run_var" + tag] + f32(EPS))]).float()


@pytest.mark.parametrize("ns,which", [(2, 1), (3, 1), (3, 2)])
@DET
@pytest.mark.parametrize("sink", [F32, F16], ids=["fp32", "fp16"])
def test_bn_bwd_finalize(sink, det, ns, which):
    key = ("bn_bwd_finalize", dname(sink) + (" det" if det else ""))
    with det_mode(det):
        for C in STATS_C:
            P = bn_params(C)
            saved = _param_saved(P)
            for T in STATS_T:
                for gscale in (1.0, 1 / 3):
                    src, buf = slot_buffer(_bwd_partials(C, ns, T), det, T)
                    B = Bufs()
                    part, gm, sv = B.put(buf), B.put(P["gamma"]), B.put(saved)
                    coef, dg, db = B.out(3 * C), B.out(C, sink), B.out(C, sink)
                    K.bn_bwd_finalize(part.view, T, ns, which, C, 577, gm.view, sv.view, coef.view,
                                      dg.view.data_ptr(), db.view.data_ptr(), gscale, sink == F16)
                    what = (C, T, gscale, ns, which, det)
                    B.check(what)
                    tot, btot = slot_total(src, det, 0 if det else -(-T // 8))
                    cref, cb = bn_bwd_coef_reference(tot[0], tot[which], 577, P["gamma"], saved, gscale, btot[0],
                                                     btot[which], sink=sink)
                    _coef_held(key, C, coef, dg, db, cref, cb, what)


# ---------------------------------------------------------------------------- backward apply
BWD_FLAGS = [pytest.mark.parametrize("dzout", [False, True], ids=["nodz", "dzout"]),
             pytest.mark.parametrize("two", [False, True], ids=["one", "two"]),
             pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])]


def _dz_bits(x, mask):
    """g [o > 0] as the kernels store it: g's own bits, +0 where masked."""
    return torch.where(x["o"].float() > 0, x["g"], torch.zeros_like(x["g"])) if mask else x["g"]


@BWD_FLAGS[0]
@BWD_FLAGS[1]
@BWD_FLAGS[2]
@DT
def test_bn_bwd_apply(dtype, mask, two, dzout):
    for C, npix in APPLY_SHAPES + ((64, 65537),):
        x, P = bn_inputs(C, npix, dtype), bn_params(C)
        k1 = (P["gamma"], P["beta"], P["gamma2"])
        k2 = (P["beta2"], P["gamma"].flip(0), P["run_mean"])
        B = Bufs()
        g, o, y1, y2 = B.put(x["g"]), B.put(x["o"]), B.put(x["y1"]), B.put(x["y2"])
        c1, c2 = B.put(torch.cat(k1)), B.put(torch.cat(k2))
        dx1, dx2, dz = B.out(npix * C, dtype), B.out(npix * C, dtype), B.out(npix * C, dtype)
        K.bn_bwd_apply(g.view, o.view if mask else None, y1.view, c1.view, dx1.view, C, y2=y2.view if two else None,
                       coef2=c2.view if two else None, dx2=dx2.view if two else None,
                       dzout=dz.view if dzout else None)
        what = (C, npix, mask, two, dzout)
        B.check(what)
        key = ("bn_bwd_apply", dname(dtype))
        ref, _, bound = bn_bwd_apply_reference(x["g"], x["o"], x["y1"], k1, mask)
        held(dx1.view, ref, bound, key, ("dx1",) + what)
        if two:
            ref, _, bound = bn_bwd_apply_reference(x["g"], x["o"], x["y2"], k2, mask)
            held(dx2.view, ref, bound, key, ("dx2",) + what)
        else:
            assert bool(torch.isnan(dx2.view).all())
        if dzout:
            assert_same_bits(dz.view, _dz_bits(x, mask).view(-1), ("dzout",) + what)
        else:
            assert bool(torch.isnan(dz.view).all())


@DET
@BWD_FLAGS[0]
@BWD_FLAGS[1]
@BWD_FLAGS[2]
@DT
def test_bn_bwd_apply_fin(dtype, mask, two, dzout, det):
    key = ("bn_bwd_apply_fin", dname(dtype) + (" det" if det else ""))
    NS = 3 if two else 2
    sink = F16 if dtype == BF16 else F32
    with det_mode(det):
        for C, npix in FIN_SHAPES:
            x, P = bn_inputs(C, npix, dtype), bn_params(C)
            s1, s2 = _param_saved(P), _param_saved(P, "2")
            src, buf = slot_buffer(_bwd_partials(C, NS, NPART, npix), det)
            B = Bufs()
            g, o, y1, y2 = B.put(x["g"]), B.put(x["o"]), B.put(x["y1"]), B.put(x["y2"])
            part, sv1, sv2, gm1, gm2 = B.put(buf), B.put(s1), B.put(s2), B.put(P["gamma"]), B.put(P["gamma2"])
            c1, dg1, db1 = B.out(3 * C), B.out(C, sink), B.out(C, sink)
            c2, dg2, db2 = B.out(3 * C), B.out(C, sink), B.out(C, sink)
            dx1, dx2, dz = B.out(npix * C, dtype), B.out(npix * C, dtype), B.out(npix * C, dtype)
            f1 = K.bn_bwd_fin(gm1.view, sv1.view, c1.view, dg1.view.data_ptr(), db1.view.data_ptr(), None, npix, 1 / 3,
                              C, sink == F16)
            f2 = K.bn_bwd_fin(gm2.view, sv2.view, c2.view, dg2.view.data_ptr(), db2.view.data_ptr(), None, npix, 1.0,
                              C, sink == F16) if two else None
            K.bn_bwd_apply_fin(g.view, o.view if mask else None, y1.view, part.view, f1, dx1.view, C,
                               y2=y2.view if two else None, fin2=f2, dx2=dx2.view if two else None,
                               dzout=dz.view if dzout else None)
            what = (C, npix, mask, two, dzout, det)
            B.check(what)
            tot, btot = slot_total(src, det)
            outs = ((1, P["gamma"], s1, c1, dg1, db1, dx1, x["y1"], 1 / 3),
                    (2, P["gamma2"], s2, c2, dg2, db2, dx2, x["y2"], 1.0))
            for which, gm, sv, c, dg, db, dx, y, gscale in outs[:NS - 1]:
                cref, cb = bn_bwd_coef_reference(tot[0], tot[which], npix, gm, sv, gscale, btot[0], btot[which],
                                                 sink=sink)
                _coef_held(key, C, c, dg, db, cref, cb, (which,) + what)
                # dx against the coefficients workgroup 0 wrote: every workgroup used the same
                kk = tuple(c.view[i * C:(i + 1) * C].cpu() for i in range(3))
                ref, _, bound = bn_bwd_apply_reference(x["g"], x["o"], y, kk, mask)
                held(dx.view, ref, bound, key, ("dx%d" % which,) + what)
            if not two:
                assert bool(torch.isnan(dx2.view).all()) and bool(torch.isnan(c2.view).all())
            if dzout:
                assert_same_bits(dz.view, _dz_bits(x, mask).view(-1), ("dzout",) + what)
            else:
                assert bool(torch.isnan(dz.view).all())


# ---------------------------------------------------------------------------- non-finite gradients
@DET
def test_nonfinite_gradient_reaches_dgamma(det):
    """Numeric inputs, not a fault: a NaN in channel 3 and an Inf in channel 12 of g (at pixels
    the mask keeps) end as NaN in that channel's dgamma / dbeta; the other channels are held to
    their bounds."""
    C, npix = 64, 577
    x, P = bn_inputs(C, npix, F32), bn_params(C)
    g, o = x["g"].clone(), x["o"].clone()
    g[5, 3], g[400, 12] = NAN, float("inf")
    o[5, 3] = o[400, 12] = 1.0
    s1, geo = true_saved(x["y1"]), reduce_geometry(npix, C)
    scale = K.det_slot_scale() if det else 1
    with det_mode(det):
        B = Bufs()
        gd, od, y1, sv, gm = B.put(g), B.put(o), B.put(x["y1"]), B.put(s1), B.put(P["gamma"])
        part = B.put(torch.zeros(SLOTS * 2 * C * scale), inout=True)
        K.bn_bwd_reduce(gd.view, od.view, y1.view, sv.view, part.view, npix, C)
        coef, dg, db, dx = B.out(3 * C), B.out(C), B.out(C), B.out(npix * C)
        f1 = K.bn_bwd_fin(gm.view, sv.view, coef.view, dg.view.data_ptr(), db.view.data_ptr(), None, npix, 1.0, C, False)
        K.bn_bwd_apply_fin(gd.view, od.view, y1.view, part.view, f1, dx.view, C)
        B.check((det,))
    bad = torch.zeros(C, dtype=torch.bool)
    bad[3] = bad[12] = True
    dgc, dbc = dg.view.cpu(), db.view.cpu()
    if det:  # poisoned entries read NaN; the float atomics carry the Inf through as it is
        assert bool(torch.isnan(dgc[bad]).all()) and bool(torch.isnan(dbc[bad]).all()), (dgc[bad], dbc[bad])
    assert not bool(torch.isfinite(dgc[bad]).any()) and not bool(torch.isfinite(dbc[bad]).any()), (dgc[bad], dbc[bad])
    g0 = g.clone()
    g0[5, 3] = g0[400, 12] = 0.0
    ref, bound = bn_bwd_sums_reference(g0, o, x["y1"], s1, None, None, True, geo, det)
    cref, cb = bn_bwd_coef_reference(ref.sum(0)[0], ref.sum(0)[1], npix, P["gamma"], s1, 1.0, bound.sum(0)[0],
                                     bound.sum(0)[1])
    ok = ~bad
    assert_within(dgc[ok], cref["dgamma"][ok], cb["dgamma"][ok], ("dgamma", det))
    assert_within(dbc[ok], cref["dbeta"][ok], cb["dbeta"][ok], ("dbeta", det))


# ---------------------------------------------------------------------------- the default path, chained
@DET
@pytest.mark.parametrize("big", [False, True], ids=["mean0", "mean100"])
@DT
def test_block_output_chain(dtype, big, det):
    """A block's output layer, o = relu(BN1(y1) + BN2(y2)), forward and backward through the
    engine's default kernels only, against torch float64 autograd of F.batch_norm. The forward
    statistics are shifted sums around k = the mean + 0.01 (the previous step's mean). The
    reference takes the kernel's ReLU mask, after checking that it agrees with the reference's own
    wherever the pre-activation is further from 0 than the forward bound.

    Measured (MI355X, error / bound and the largest |dx1| error): see profiles/bn_paths.txt."""
    C, npix = CHAIN
    x, P = bn_inputs(C, npix, dtype, big_mean=big), bn_params(C)
    gscale, sink = 1 / 3, F32
    geo = reduce_geometry(npix, C)
    scale = K.det_slot_scale() if det else 1
    tag = dname(dtype) + (" mean100" if big else " mean0") + (" det" if det else "")
    ks = [(x[n].double().mean(0) + 0.01).float() for n in ("y1", "y2")]
    with det_mode(det):
        B = Bufs()
        y1, y2, g = B.put(x["y1"]), B.put(x["y2"]), B.put(x["g"])
        srcs, parts, fins, affs, savs, gms = [], [], [], [], [], []
        for i, (yn, t) in enumerate((("y1", ""), ("y2", "2"))):
            src, buf = _fwd_slots(x[yn], det, ks[i])
            srcs.append(src)
            parts.append(B.put(buf))
            gms.append(B.put(P["gamma" + t]))
            affs.append(B.out(2 * C))
            savs.append(B.out(2 * C))
            fins.append(K.bn_fin(gms[i].view, B.put(P["beta" + t]).view, None, None, affs[i].view, savs[i].view, None,
                                 npix, EPS, MOMENTUM, C, sshift=B.put(ks[i]).view))
        o = B.out(npix * C, dtype)
        K.bn_apply_fin(y1.view, parts[0].view, fins[0], o.view, C, relu=True, res=y2.view, part2=parts[1].view,
                       fin2=fins[1])
        bpart = B.put(torch.zeros(SLOTS * 3 * C * scale), inout=True)
        K.bn_bwd_reduce(g.view, o.view, y1.view, savs[0].view, bpart.view, npix, C, y2=y2.view, saved2=savs[1].view)
        coefs, dgs, dbs, dxs, bfs = [], [], [], [], []
        for i in range(2):
            coefs.append(B.out(3 * C))
            dgs.append(B.out(C))
            dbs.append(B.out(C))
            dxs.append(B.out(npix * C, dtype))
            bfs.append(K.bn_bwd_fin(gms[i].view, savs[i].view, coefs[i].view, dgs[i].view.data_ptr(),
                                    dbs[i].view.data_ptr(), None, npix, gscale, C, False))
        dz = B.out(npix * C, dtype)
        K.bn_bwd_apply_fin(g.view, o.view, y1.view, bpart.view, bfs[0], dxs[0].view, C, y2=y2.view, fin2=bfs[1],
                           dx2=dxs[1].view, dzout=dz.view)
        B.check((tag,))
    # ---- reference: float64 autograd
    eps = f32(EPS)
    yd = [x[n].double().requires_grad_() for n in ("y1", "y2")]
    gam = [P[n].double().requires_grad_() for n in ("gamma", "gamma2")]
    bet = [P[n].double().requires_grad_() for n in ("beta", "beta2")]
    t = sum(F.batch_norm(yd[i], None, None, gam[i], bet[i], True, 0.0, eps) for i in range(2))
    # forward: the exact batch statistics; the slots hold host partials rounded to fp32 once each
    # (u / 2 of each partial, and as much again for a float row of two or three of them)
    st, exact, b_o = [], [], 0.0
    for i, s in enumerate(("", "2")):
        partials = stats_slots(x["y%d" % (i + 1)], SLOTS, ks[i], nparts=NPART)
        ref, bd = bn_stats_reference(srcs[i], npix, ks[i], P["gamma" + s], P["beta" + s], EPS, MOMENTUM, None, None,
                                     det=det, b_slots=U * partials.double().abs().sum(0))
        d = yd[i].detach()
        mean = d.mean(0)
        ex = dict(mean=mean, invstd=1.0 / torch.sqrt(((d - mean) ** 2).mean(0) + eps))
        st.append((ref, bd))
        exact.append(ex)
        held(savs[i].view[:C], ex["mean"], bd["mean"], ("chain saved mean", tag), (i,))
        held(savs[i].view[C:], ex["invstd"], bd["invstd"], ("chain saved invstd", tag), (i,))
        b_o = b_o + d.abs() * bd["scale"] + bd["shift"]
    sc = [gam[i].detach() * exact[i]["invstd"] for i in range(2)]
    sh = [bet[i].detach() - exact[i]["mean"] * sc[i] for i in range(2)]
    oref, b_apply = bn_apply_reference(x["y1"], sc[0], sh[0], x["y2"], sc[1], sh[1], True, 2)
    b_o = b_o + b_apply
    held(o.view, oref, b_o, ("chain o", tag), ())
    o_cpu = o.view.cpu().view(npix, C)
    mask = (o_cpu.float() > 0)
    sure = t.detach().abs() > b_o
    assert bool((mask == (t.detach() > 0))[sure].all()), "the ReLU mask differs where the bound decides it"
    (t * mask.double() * x["g"].double()).sum().backward()
    assert_same_bits(dz.view, torch.where(mask, x["g"], torch.zeros_like(x["g"])).view(-1), ("dz", tag))
    # backward sums with the exact statistics; the kernel's saved ones are within b(mean), b(invstd)
    svx = [torch.stack([exact[i]["mean"], exact[i]["invstd"]]) for i in range(2)]
    sums, bsum = bn_bwd_sums_reference(x["g"], o_cpu, x["y1"], svx[0], x["y2"], svx[1], True, geo, det)
    tot, btot = sums.sum(0), bsum.sum(0)
    dzabs = (x["g"].double() * mask.double()).abs()
    for i in range(2):
        bm, bi = st[i][1]["mean"], st[i][1]["invstd"]
        d = yd[i].detach()
        b_x = (dzabs * (bm * svx[i][1] + (d - svx[i][0]).abs() * bi)).sum(0)
        cref, cb = bn_bwd_coef_reference(tot[0], tot[1 + i], npix, gam[i].detach(), svx[i], gscale, btot[0],
                                         btot[1 + i] + b_x, b_mean=bm, b_is=bi)
        _coef_held(("chain coef", tag), C, coefs[i], dgs[i], dbs[i], cref, cb, (i,))
        held(dgs[i].view, gam[i].grad * f32(gscale), cb["dgamma"], ("chain dgamma (autograd)", tag), (i,))
        held(dbs[i].view, bet[i].grad * f32(gscale), cb["dbeta"], ("chain dbeta (autograd)", tag), (i,))
        dx, _, bdx = bn_bwd_apply_reference(x["g"], o_cpu, x["y%d" % (i + 1)], (cref["k1"], cref["k2"], cref["k3"]),
                                            True, (cb["k1"], cb["k2"], cb["k3"]), out_dtype=dtype)
        # the formula is the gradient: float64 autograd agrees with it far inside the bound
        assert bool(((dx - yd[i].grad).abs() <= 1e-3 * bdx + 1e-300).all()), (tag, i)
        err = (dxs[i].view.cpu().double().view(npix, C) - yd[i].grad).abs()
        FIGURES["chain dx%d %s: max |error| (max |dx| %.3g)" % (i + 1, tag, float(yd[i].grad.abs().max()))] = \
            "%.3e" % float(err.max())
        held(dxs[i].view, yd[i].grad, bdx, ("chain dx", tag), (i,))
