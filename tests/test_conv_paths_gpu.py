"""The conv v2 kernels of csrc/kernels/conv_v2.hip, directly, on every dispatch path, bit for bit
against the fp64 references of tests/test_conv_cpu.py (exact integer operands: no tolerance), plus
one random-operand case per path inside the per-element bound stated there.

Every launch (launch_case): K.conv2_path must first report the path the case names (under the
case's PSX_TUNE, set before the workspace query and the launch); every buffer lies between
canaries (Placed); the output and the split-K workspace are pre-filled with NaN, the slot buffers
zeroed as the engine does; afterwards the canaries are intact, the inputs unchanged bit for bit,
every output element equals the reference and EVERY SLOT ROW equals its own reference.

Which test reaches which branch (the case tables live in tests/test_conv_cpu.py):

  conv2_kernel generic mainloop, MODE 0 / 1      test_exact[generic-*]
    gather_src (log2_icc < 3), fwd s1 / s2       gather-ic*-s1 / -s2 (5x7, N 2)
    zero-padded k columns, tap >= R S            stem7 (7x7 s2 p3, 19x17, Kg 392 -> 448 / 196 -> 224)
    gather_src, MODE 1                           dgrad-gather[-res]
    uniform tap: s2 p1, s2 p0, 1x1 s2            utap-s2p1 (9x7), utap-s2p0 (7x9), utap-1x1s2 (9x7)
    gemm1x1 shortcut, 75 and 35 pixels           gemm1x1-75 (+ fuse_fin), gemm1x1-35
    ring with 1, 2, 3, 4, 9 k-steps + statistics ring1, ring2 (+ sshift), ring4, ring9; three k-steps:
                                                 gather-ic16-*-bf16 / gather-ic8-*-f32 (Kg 144 -> 192 /
                                                 72 -> 96, kps = 3 pinned), per split in splitk4-*
    every dispatch2 tile, 75 px and 3 tiles      tile{BM}x{BN}x{WGM}-75 / -3t, fwd + statistics and
                                                 dgrad + residual + bst
    dgrad with / without residual, bst           dgrad-1x1[-res], dgrad-3x3[-res]
  MODE 2 (stride-2 dgrad, forward OC < 64)       test_exact[mode2-*]: OC 8/16/32 (fp32 4/8/16), 3x3 p1
                                                 and 1x1 p0, dx 9x7 (+ residual) and 8x8
  MODE 3 (parity classes)                        test_exact[parity-*]: OC 64 / 128, 3x3 and 1x1, dx
                                                 8x8, 9x7, 7x7, 1x1 (empty classes return early), 2x1;
                                                 residual, bst 2 / 3, mask_store rotate over the sizes;
                                                 1x1 / s2: the tapless classes write 0 + res
    7x7 s2 p3                                    parity-7x7
    class (0,0) one more tile than (1,1)         parity-tiles (9x15, N 2: 80 and 56 pixels)
    64x64 / 64x128 class tiles                   parity-* (64x64: the planner's choice at these sizes),
                                                 parity-64x128 (forced with cv_bn=128: the planner picks
                                                 it only from 512 tiles on, far more pixels than here)
    shortcut fold (conv_dgrad2_sc)               fold-* (+ bst 2 / 3, mask_store); test_fold_refusals
  tap reuse, whole rows                          test_exact[tapr-*]: W = H in 1 .. 64 (W 4: four
                                                 images per tile), IC 64 / 128, fwd + statistics /
                                                 sshift / fuse_fin, dgrad + residual / bst / mask_store
    128- and 256-pixel tiles                     tapr-bn128-*, tapr-bn256-* (cv_tapr_bn)
  tap reuse, halo                                test_exact[halo-*]: 7x7 (147 px), 5x7 (35 px), 14x14,
                                                 1x9, 9x1, forced on 70 x 1x1 and on 8x8 (128 px)
    cv_tapr_halo=0 falls to the generic path     test_halo_off_agrees (bit for bit with the halo result)
  split-K + conv_splitk_epilogue                 test_exact[splitk-*]: natural (IC 128 / 64, 3x3 s2),
                                                 cv_splits 2 / 4 (last split empty) / 8 (splits past
                                                 the end), 1 / 33 / 160 pixels, OC 64 and 2048; fwd +
                                                 statistics / sshift / fuse_fin, dgrad + residual / bst
                                                 / mask_store
    -8 (OC 192), -9 (no workspace), -2           test_split_refusals
  no statistics and no BN-backward sums          test_exact[plain-*]: forward on the generic (gather,
    (the early exits `if (!st && !bwd) return`   uniform tap, gemm1x1, three tiles), tap-reuse (64- and
    of conv2_kernel and conv_splitk_epilogue)    128-pixel tiles), halo (147 and 35 px) and split-K paths
                                                 (natural, cv_splits=2 at 33 / 160 px); split-K dgrad with
                                                 and without residual (cv_splits 2 and 4)
  deterministic mode, every epilogue kind        test_exact[det-*]: slot words equal the host
                                                 encoder's, two launches identical, fuse_fin of the
                                                 decoded slots
  fuse_fin (bnfin.hpp last_block_arrive)         every case with fin (gemm1x1-75, tapr-w8-fwd, halo-3x7x7-
                                                 fwd, splitk2-*-fwd, det-generic-fwd, det-splitk-fwd): the
                                                 BN outputs against bn_stats_reference of the slots the
                                                 launch wrote; again after the engine's re-zeroing of slots
                                                 and counter: the same bits; then once more on the counter
                                                 left as it is: nothing is finalized (check_no_fin)
  psx_bgemm_f32 / _split (2-deep ring)           test_bgemm_f32: cfg 0-3, nb 1 / 2 / 6, s2 1 / 2, Kd 32 /
                                                 64 / 128, M 35 / 64 / 150, N 64 / 128; test_bgemm_refusals
  accuracy class, bf16 rounding of non-integers  test_numerics (ratios printed by _report)
  K.param_unpack against build_wf / build_wd     test_param_unpack_matches_host_layout
"""
import math
import time

import pytest
import torch

from psx.ops import kernels as K
from psx.ops._lib import HipError

from .test_bn_cpu import EPS, MOMENTUM, SLOTS, bn_stats_reference, fix_encode_tensor
from .test_conv_cpu import (ALL_EXACT, BF16, EXACT_TABLES, F32, NUMERICS, build_wd, build_wf, case_data, ids, nhwc,
                            query_path, slot_total_bound, workgroup_of)
from .test_sgd_cpu import assert_within
from .test_sgd_gpu import DEV, Placed, assert_same_bits

pytestmark = pytest.mark.gpu

RATIOS, COUNTS = {}, {}
T0 = time.time()
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(RATIOS):
        print("conv_paths ratio", *key, "%.4f" % RATIOS[key])
    for key in sorted(COUNTS):
        print("conv_paths exact cases", key, COUNTS[key])
    print("conv_paths wall seconds %.1f" % (time.time() - T0))


def _flat(t, dtype):
    return t.to(dtype).reshape(-1).contiguous()


def _nan(n, dtype):
    return torch.full((n,), NAN, dtype=dtype)


class Launch:
    """The placed buffers of one case and its launch (see the module docstring)."""

    def __init__(self, case, d, path):
        c, T = case, case.dtype
        self.c, self.d, self.path = c, d, path
        C = c.out_shape[-1]
        self.C, self.npix = C, c.out_shape[0] * c.out_shape[1] * c.out_shape[2]
        self.inputs = {"act": Placed(_flat(nhwc(d["act"]), T)), "w": Placed(_flat(d["wmat"], T))}
        if c.res:
            self.inputs["res"] = Placed(_flat(d["res"], T))
        if c.dir == "dgrad_sc":
            self.inputs["act_sc"] = Placed(_flat(nhwc(d["dy_sc"]), T))
            self.inputs["w_sc"] = Placed(_flat(d["wmat_sc"], T))
        if c.sshift:
            self.inputs["sshift"] = Placed(d["sshift"].float())
        if c.bst:
            for k in ("o", "y1", "y2"):
                if d[k] is not None:
                    self.inputs[k] = Placed(_flat(d[k], T))
            self.inputs["saved1"] = Placed(_flat(d["saved1"], F32))
            if d["saved2"] is not None:
                self.inputs["saved2"] = Placed(_flat(d["saved2"], F32))
        self.out = Placed(_nan(self.npix * C, T))
        oh, ow = c.out_shape[1:3]
        wsb = K.conv2_workspace_bytes(c.n, oh, ow, C, c.kg, c.f32)
        split = path["splits"] > 1 and path["mode"] != 3
        if path["kind"] == "generic" and path["mode"] != 3:  # the query plans the generic path only
            assert wsb == (path["splits"] * self.npix * C * 4 if split else 0), (c.id, wsb, path)
        self.ws = Placed(_nan(path["splits"] * self.npix * C, F32)) if split else None
        self.ns = 2 if c.stats else c.bst
        self.slots = Placed(torch.zeros(SLOTS * self.ns * C * (4 if c.det else 1))) if self.ns else None
        self.fin = None
        if c.fin:
            g = torch.Generator().manual_seed(c.seed + 7)
            self.fin0 = dict(gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g),
                             run_mean=torch.randn(C, generator=g), run_var=torch.rand(C, generator=g) + 0.5)
            self.inputs["gamma"], self.inputs["beta"] = Placed(self.fin0["gamma"]), Placed(self.fin0["beta"])
            self.fout = {k: Placed(_nan(n, F32)) for k, n in (("affine", 2 * C), ("saved", 2 * C), ("sshift_next", C))}
            self.fout["run_mean"], self.fout["run_var"] = Placed(self.fin0["run_mean"]), Placed(self.fin0["run_var"])
            self.counter = Placed(torch.zeros(64))

    def placed(self):
        extra = [self.out, self.ws, self.slots] + (list(self.fout.values()) + [self.counter] if self.c.fin else [])
        return list(self.inputs.values()) + [p for p in extra if p is not None]

    def reset(self, counter=True):
        """What the engine does between steps: slots and counters zeroed; here also NaN outputs.
        ``counter=False`` leaves the arrival counter as the last launch left it."""
        self.out.view.fill_(NAN)
        for p in (self.slots, self.counter if self.c.fin and counter else None):
            if p is not None:
                p.view.zero_()
        if self.ws is not None:
            self.ws.view.fill_(NAN)
        if self.c.fin:
            for k in ("affine", "saved", "sshift_next"):
                self.fout[k].view.fill_(NAN)
            for k in ("run_mean", "run_var"):
                self.fout[k].view.copy_(self.fin0[k])

    def run(self):
        c, v = self.c, {k: p.view for k, p in self.inputs.items()}
        ws = self.ws.view if self.ws is not None else None
        slots = self.slots.view if self.slots is not None else None
        if c.dir == "fwd":
            fin = None
            if c.fin:
                fin = K.bn_fin(v["gamma"], v["beta"], self.fout["run_mean"].view, self.fout["run_var"].view,
                               self.fout["affine"].view, self.fout["saved"].view, self.counter.view.data_ptr(),
                               self.npix, EPS, MOMENTUM, self.C, sshift=v.get("sshift"),
                               sshift_next=self.fout["sshift_next"].view)
            K.conv_fwd2(v["act"], v["w"], self.out.view, slots if c.stats else None, ws, c.n, c.h, c.w, c.ic, c.oc, c.k,
                        c.stride, c.pad, c.kg, fin=fin, sshift=v.get("sshift"))
        else:
            bst = None
            if c.bst:
                bst = K.bwd_stats_desc(slots, v["o"], v["y1"], v["saved1"], v.get("y2"), v.get("saved2"),
                                       mask_store=c.mask)
            if c.dir == "dgrad_sc":
                assert K.conv_dgrad2_sc(v["act"], v["w"], self.out.view, ws, c.n, c.h, c.w, c.ic, c.oc, c.kg,
                                        v["act_sc"], v["w_sc"], c.oc, bst=bst)
            else:
                K.conv_dgrad2(v["act"], v["w"], self.out.view, v.get("res"), ws, c.n, c.h, c.w, c.ic, c.oc, c.k,
                              c.stride, c.pad, c.kg, bst=bst)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:  # a GPU fault: nothing more may run on this device
            pytest.exit(f"GPU fault in {c.id}: {e}", returncode=3)

    def check_memory(self):
        for p in self.placed():
            assert p.intact(), (self.c.id, "canary overwritten")
        for k, p in self.inputs.items():
            assert p.unchanged(), (self.c.id, "input changed", k)

    def slot_values(self):
        """The slot rows [8][NS][C] as float64 (decoded in deterministic mode)."""
        shape = (SLOTS, self.ns, self.C)
        if self.c.det:
            return K.det_slot_values(self.slots.view, shape).cpu()
        return self.slots.view.view(*shape).cpu().double()

    def slot_words(self):
        n = SLOTS * self.ns * self.C
        return self.slots.view.view(torch.int64)[:2 * n].view(SLOTS, self.ns, self.C, 2).cpu().clone()

    def check_fin(self):
        """The fuse_fin outputs against bn_stats_reference of the slots this launch wrote."""
        c, C = self.c, self.C
        assert int(self.counter.view.view(torch.int32)[0]) > 0 and not self.counter.view[1:].any()
        slots = self.slot_words() if c.det else self.slots.view.view(SLOTS, 2, C).cpu()
        f0 = self.fin0
        ref, bound = bn_stats_reference(slots, self.npix, self.d.get("sshift"), f0["gamma"], f0["beta"], EPS, MOMENTUM,
                                        f0["run_mean"], f0["run_var"], det=c.det)
        aff, sav = self.fout["affine"].view.cpu().view(2, C), self.fout["saved"].view.cpu().view(2, C)
        got = dict(scale=aff[0], shift=aff[1], mean=sav[0], invstd=sav[1],
                   sshift_next=self.fout["sshift_next"].view.cpu(),
                   run_mean=self.fout["run_mean"].view.cpu(), run_var=self.fout["run_var"].view.cpu())
        for k, x in got.items():
            assert_within(x, ref[k], bound[k], (c.id, "fuse_fin", k))
        return {k: x.clone() for k, x in got.items()}

    def arrivals(self):
        return int(self.counter.view.view(torch.int32)[0])

    def check_no_fin(self, arrivals):
        """After a launch on a counter that was not re-zeroed: its workgroups drew the tickets
        arrivals .. 2 arrivals - 1, none of them the last of a fresh count, so nothing was
        finalized: the NaN-filled BN outputs and the running statistics are untouched."""
        assert self.arrivals() == 2 * arrivals, (self.c.id, "arrival counter", self.arrivals(), arrivals)
        for k in ("affine", "saved", "sshift_next"):
            assert bool(torch.isnan(self.fout[k].view).all()), (self.c.id, "finalized on a stale counter", k)
        for k in ("run_mean", "run_var"):
            assert_same_bits(self.fout[k].view, self.fin0[k], (self.c.id, "finalized on a stale counter", k))


def det_words(d, path, key, C, out_shape):
    """The deterministic-mode words the host encoder gives for the per-workgroup partial totals."""
    c = d["case"]
    from .test_conv_cpu import bwd_terms
    if key == "stats_ref":
        dd = d["stored"].double().reshape(-1, C) - (d["sshift"].double() if d.get("sshift") is not None else 0.0)
        terms = torch.stack([dd, dd * dd])
    else:
        g = d["ref"].float().to(c.dtype)  # the stored gradient before mask_store
        terms = bwd_terms(g, d["o"], d["y1"], d["saved1"], d["y2"], d["saved2"])
    wg, nwg = workgroup_of(path, *out_shape[:3])
    part = torch.zeros(nwg, terms.shape[0], C, dtype=torch.float64)
    for k in range(terms.shape[0]):
        part[:, k].index_add_(0, wg, terms[k])
    row_of = torch.zeros(nwg, dtype=torch.long)
    row_of[wg] = d["rows"]
    pair, bad = fix_encode_tensor(part.float())
    assert not bool(bad.any())
    out = torch.zeros(SLOTS, terms.shape[0], C, 2, dtype=torch.int64)
    out.index_add_(0, row_of, pair)
    return out


def launch_case(case, monkeypatch, numerics=False):
    path = query_path(case, monkeypatch)
    d = case_data(case, path, numerics)
    L = Launch(case, d, path)
    if case.det:
        K.set_deterministic(True)
    try:
        L.run()
        L.check_memory()
        out = L.out.view.cpu().clone()
        slots = L.slot_values() if L.ns else None
        again = None
        if case.fin or case.det:
            words = L.slot_words() if case.det else None
            fin = L.check_fin() if case.fin else None
            L.reset()
            L.run()
            L.check_memory()
            assert_same_bits(L.out.view, out, (case.id, "second launch"))
            if case.det:
                assert torch.equal(L.slot_words(), words), (case.id, "deterministic words differ between two launches")
                key = "stats_ref" if case.stats else "bsums_ref"
                want = det_words(d, path, key, L.C, case.out_shape)
                assert torch.equal(words, want), (case.id, "host encoder's words")
            if case.fin:
                again = L.check_fin()
                for k in fin:
                    assert_same_bits(again[k], fin[k], (case.id, "fuse_fin after re-zeroing", k))
                n1 = L.arrivals()
                L.reset(counter=False)
                L.run()
                L.check_memory()
                assert_same_bits(L.out.view, out, (case.id, "launch on a stale counter"))
                L.check_no_fin(n1)
    finally:
        if case.det:
            K.set_deterministic(False)
    return L, d, path, out, slots


def path_key(case, path):
    kind = path["kind"] if path["splits"] == 1 else "splitk"
    return (kind if path["mode"] < 2 else f"mode{path['mode']}", case.dir.split("_")[0], "f32" if case.f32 else "bf16")


def check_exact(case, monkeypatch, count=True):
    L, d, path, out, slots = launch_case(case, monkeypatch)
    assert_same_bits(out, d["stored"].reshape(-1), (case.id, "output"))
    if L.ns:
        ref = d["stats_ref"] if case.stats else d["bsums_ref"]
        ne = slots != ref
        assert not bool(ne.any()), (case.id, "slot entries that differ", int(ne.sum()), "first (row, sum, channel)",
                                    ne.nonzero()[0].tolist(), float(slots[ne][0]), float(ref[ne][0]))
    if count:
        key = path_key(case, path)
        COUNTS[key] = COUNTS.get(key, 0) + 1
    return out


EXACT_RUN = [c for name, tab in EXACT_TABLES.items() if name != "halo_off" for c in tab]


@pytest.mark.parametrize("case", EXACT_RUN, ids=ids(EXACT_RUN))
def test_exact(case, monkeypatch):
    check_exact(case, monkeypatch)


HALO_PAIRS = list(zip(EXACT_TABLES["halo"], EXACT_TABLES["halo_off"]))


@pytest.mark.parametrize("on,off", HALO_PAIRS, ids=[c.id for c, _ in HALO_PAIRS])
def test_halo_off_agrees(on, off, monkeypatch):
    """cv_tapr_halo=0 (cv_tapr=0 where the halo mode was forced): the same launch takes the generic
    path, equals its own references, and its output equals the halo launch's bit for bit."""
    a = check_exact(off, monkeypatch)
    b = check_exact(on, monkeypatch, count=False)
    assert_same_bits(a, b, (on.id, "halo against generic"))


def _ratio(x, ref, bound):
    return float(((x.double() - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf).max())


@pytest.mark.parametrize("case", NUMERICS, ids=ids(NUMERICS))
def test_numerics(case, monkeypatch):
    """Random bf16-representable operands: every output inside its element bound, the slot totals
    inside the any-order bound of the sums of the values the kernel itself stored."""
    from .test_conv_cpu import fwd_stats_reference
    L, d, path, out, slots = launch_case(case, monkeypatch, numerics=True)
    key = path_key(case, path)
    ref, bound = d["ref"].reshape(-1), d["bound"].reshape(-1)
    RATIOS[key + ("out",)] = _ratio(out, ref, bound)
    print("conv_paths numerics", case.id, "out", RATIOS[key + ("out",)])
    assert_within(out, ref, bound, (case.id, "output"))
    if case.stats:
        stored = out.view(case.out_shape)
        tot = fwd_stats_reference(stored, d["rows"], d["sshift"]).sum(0)
        b = slot_total_bound(d, "stats_ref", stored=stored)
        RATIOS[key + ("slots",)] = _ratio(slots.sum(0), tot, b)
        print("conv_paths numerics", case.id, "slots", RATIOS[key + ("slots",)])
        assert_within(slots.sum(0).reshape(-1), tot.reshape(-1), b.reshape(-1), (case.id, "slot totals"))


def _code(fn, *a, **kw):
    with pytest.raises(HipError) as e:
        fn(*a, **kw)
    return int(str(e.value).rsplit(" ", 1)[1])


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_split_refusals(f32, monkeypatch):
    """-8: the epilogue's 256 % (OC / 8) (OC 192; the split launches ran, the epilogue did not: the
    output stays NaN); -9: a split plan and no workspace, -2: IC no power of two (both before any
    launch: the output stays NaN)."""
    T, ks = (F32 if f32 else BF16), (32 if f32 else 64)
    n, h, w = 1, 5, 7
    monkeypatch.setenv("PSX_TUNE", "cv_splits=2,cv_tapr=0")

    def go(ic, oc, ws):
        kg = -(-9 * ic // ks) * ks
        x, wf = Placed(torch.zeros(n * h * w * ic, dtype=T)), Placed(torch.zeros(oc * kg, dtype=T))
        y = Placed(_nan(n * h * w * oc, T))
        wsp = Placed(_nan(2 * n * h * w * oc, F32)) if ws else None
        rc = _code(K.conv_fwd2, x.view, wf.view, y.view, None, wsp.view if ws else None, n, h, w, ic, oc, 3, 1, 1, kg)
        torch.cuda.synchronize()
        assert all(p.intact() for p in (x, wf, y) + ((wsp,) if ws else ()))
        assert bool(torch.isnan(y.view.float()).all()), "a refused launch wrote the output"
        return rc

    assert K.conv2_path("fwd", n, h, w, ks, 192, 3, 1, 1, 9 * ks, f32)["splits"] == 2
    assert go(ks, 192, True) == -8
    assert go(ks, 64, False) == -9
    assert K.conv2_path("fwd", n, h, w, 48, 64, 3, 1, 1, -(-9 * 48 // ks) * ks, f32) == -2
    assert go(48, 64, True) == -2


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_fold_refusals(f32, monkeypatch):
    """psx_conv_dgrad2_sc returns -11 and launches nothing: with a residual, for a layer that is
    not 3x3 / s2 / p1, with Kg_sc != OC_fwd, and with a forward OC below 64 (no parity path)."""
    from psx.ops._lib import kernels, ptr, stream_ptr
    monkeypatch.delenv("PSX_TUNE", raising=False)
    T, ks = (F32 if f32 else BF16), (32 if f32 else 64)
    n, h, w, ic = 2, 9, 7, 64

    def go(oc, k, stride, pad, res, kg_sc):
        P, Q = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        kg = -(-k * k * oc // ks) * ks
        dy, dy2 = (Placed(torch.zeros(n * P * Q * oc, dtype=T)) for _ in range(2))
        wd, wd2 = Placed(torch.zeros(ic * kg, dtype=T)), Placed(torch.zeros(ic * max(kg_sc, ks), dtype=T))
        r = Placed(torch.zeros(n * h * w * ic, dtype=T))
        dx = Placed(_nan(n * h * w * ic, T))
        rc = kernels().psx_conv_dgrad2_sc(ptr(dy.view), ptr(wd.view), ptr(dx.view), ptr(r.view) if res else None,
                                          ptr(K.zero_page(DEV)), None, n, h, w, ic, oc, k, k, stride, pad, kg, None,
                                          int(f32), ptr(dy2.view), ptr(wd2.view), kg_sc, stream_ptr())
        torch.cuda.synchronize()
        assert all(p.intact() for p in (dy, dy2, wd, wd2, r, dx))
        assert bool(torch.isnan(dx.view.float()).all()), "a refused launch wrote the output"
        return rc

    assert go(64, 3, 2, 1, True, 64) == -11
    assert go(64, 1, 2, 0, False, 64) == -11
    assert go(64, 3, 1, 1, False, 64) == -11
    assert go(64, 3, 2, 1, False, 128) == -11
    low = 16 if f32 else 32
    assert K.conv2_path("dgrad_sc", n, h, w, ic, low, 3, 2, 1, -(-9 * low // ks) * ks, f32) == -11
    assert go(low, 3, 2, 1, False, low) == -11


BGEMM = [(nb, s2, kd) for nb, s2 in ((1, 2), (2, 1), (6, 1), (2, 2)) for kd in (32, 64, 128) if (kd // 32) % s2 == 0]


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("nb,s2,kd", BGEMM, ids=[f"nb{a}-s{b}-kd{c}" for a, b, c in BGEMM])
def test_bgemm_f32(nb, s2, kd, cfg):
    """psx_bgemm_f32 / psx_bgemm_f32_split: the conv mainloop's 2-deep ring with 1, 2 and 4 k-steps
    per slab (Kd / 32 / s2), every tile configuration, M below one tile, one tile and three tiles
    with a partial last: exact integer operands, bit for bit against fp64, NaN-filled slabs."""
    gen = torch.Generator().manual_seed(nb * 100 + s2 * 10 + cfg)
    for M in (35, 64, 150):
        for N in (64, 128):
            A = torch.randint(-3, 4, (nb, M, kd), generator=gen).double()
            B = torch.randint(-2, 3, (N, nb, kd), generator=gen).double()
            r = kd // s2
            ranges = [(b, slice(j * r, (j + 1) * r)) for b in range(nb) for j in range(s2)]
            ref = torch.stack([A[b, :, ks] @ B[:, b, ks].t() for b, ks in ranges])
            a, b_, p = Placed(_flat(A, F32)), Placed(_flat(B, F32)), Placed(_nan(nb * s2 * M * N, F32))
            if s2 == 1:
                K.bgemm_f32(a.view, b_.view, p.view, M, N, kd, nb, cfg)
            else:
                assert K.bgemm_f32_split(a.view, b_.view, p.view, M, N, kd, nb, s2, cfg) == 0
            torch.cuda.synchronize()
            assert a.intact() and b_.intact() and p.intact() and a.unchanged() and b_.unchanged()
            assert_same_bits(p.view, ref.float().reshape(-1), ("bgemm", nb, s2, kd, cfg, M, N))
    COUNTS[("bgemm", "f32")] = COUNTS.get(("bgemm", "f32"), 0) + 6


def test_bgemm_refusals():
    """The documented -2 refusals, before any launch: N % 64, Kd below 32 or no power of two, s2 not
    dividing the k-steps, one slab in all."""
    a, b, p = (Placed(torch.zeros(6 * 150 * 128)) for _ in range(3))
    p.view.fill_(NAN)
    for M, N, kd, nb, s2 in ((64, 96, 64, 2, 1), (64, 64, 16, 2, 1), (64, 64, 96, 2, 1), (64, 64, 64, 2, 3), (64, 64,
                                                                                                              64, 1, 1),
                             (0, 64, 64, 2, 1)):
        assert K.bgemm_f32_split(a.view, b.view, p.view, M, N, kd, nb, s2, 0) == -2, (M, N, kd, nb, s2)
    torch.cuda.synchronize()
    assert p.intact() and bool(torch.isnan(p.view).all())


@pytest.mark.parametrize("shape", [(64, 8, 3), (64, 5, 3), (64, 64, 1), (64, 3, 7)], ids=lambda s: "x".join(map(str,
                                                                                                                s)))
def test_param_unpack_matches_host_layout(shape):
    """K.param_unpack of an OIHW tensor equals the host-built wf / wd bit for bit (3x3 at IC 8 and 5:
    a padded Kg, and padded channels; a 1x1; the 7x7 stem: Kg 392 -> 448)."""
    from .test_kernels_gpu import make_operands
    oc, cin, k = shape
    w = torch.randn(oc, cin, k, k, generator=torch.Generator().manual_seed(3)).to(BF16).float()
    wf, wd, cp, kg, kgd = make_operands(w.to(DEV))
    wp = torch.zeros(oc, cp, k, k)
    wp[:, :cin] = w
    hf, hd = build_wf(wp, 64), build_wd(wp, 64)
    assert hf.shape == (oc, kg) and hd.shape == (cp, kgd)
    assert_same_bits(wf, hf.to(BF16).reshape(-1), "wf")
    assert_same_bits(wd, hd.to(BF16).reshape(-1), "wd")


