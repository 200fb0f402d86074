"""The classifier head kernels of csrc/kernels/head.hip, directly, against the fp64 references and
the bounds of tests/test_head_cpu.py, on every path: both storage types, the fused per-sample
kernel and the split path, training and eval, deterministic mode off and on, both gradient sinks.
Every buffer a kernel sees lies inside a larger allocation of canaries; outputs are pre-filled with
NaN, inputs are checked unchanged; every element is held to its own bound. Shapes are (B, HW, C, K).

Which test reaches which branch:

  psx_head_fwd_bwd
    head_split false, fused ok   test_head_forward_backward, FUSED rows
      head_kernel<T, true>       T = uint16_t / float by the dtype parameter
        pooling loop             no thread's second trip, 8 threads busy: (1, 1, 16, 1); all 256 threads once:
                                 (9, 16, 512, 100); second trip: (5, 4, 1024, 100)
        class-row loop           one trip, 1 / 10 / 100 rows: the first three rows of the table; fifth trip
                                 (K > 256): (19, 4, 256, 257); all sixteen: (2, 1, 256, 1024), K C = 2^18,
                                 the last fused size and the K the header now states
        argmax                   kind tie: equal maxima in different lanes (K 100: rows 20, 50, 99) and in one
                                 lane (K 257: rows 128 and 256 are lane 0); the label is the lowest, a middle
                                 or an untied row, so the count tells the lowest from any other choice
        max subtraction          kind wide: logits over +-40, most exps underflow towards 0
        labels 0 and K - 1       kind edge_labels
        pooled null              test_head_null_buffers_take_the_fused_kernel (2, 1, 512, 1000): head_split
                                 false only for the null buffer
        bst given / not          first / second launch of test_head_forward_backward; the returned flag equals
                                 psx_head_sums_ok; the sums: test_head_bn_sums
        HeadBnStats, stat_add    test_head_bn_sums[dtype-float / det]: B in 1, 8, 9, 19 (one row; every row
                                 once; row 0 twice; rows 0 - 2 three times) at (4, 64, 10), and (9, 4, 1024,
                                 100) (second channel trip); every slot row held to its own bound
      head_kernel<T, false>      test_head_eval, FUSED rows: dlogits and dact untouched; loss null; correct null
      bst with dact null         test_head_bn_sums: returns false, part untouched
    head_fused_ok false: -2      test_head_refusals: (C 16, K 1025), (C 24, K 10), (C 768, K 10); also on the
                                 host in tests/test_head_cpu.py
    head_split true              test_head_forward_backward / test_head_eval, SPLIT rows
      head_pool_kernel<T>        one channel block (C 320, 64: threads past C return), two (C 1024, 768);
                                 HW 1, 4, 49; zeroes B K logits with B K from 264 to 27,753
      head_gemm_kernel<true, 0>  ks 4 with a short last range, K % 4 = 1 (the n + j < N tail), two sample
                                 tiles with one row in the second: (33, 4, 320, 841); ks 16, B 1, HW 1:
                                 (1, 1, 1024, 264); K > 1024, two of four ranges empty: (2, 4, 64, 4104); a C
                                 the fused kernel refuses: (3, 49, 768, 400); ks 1: every row in det mode,
                                 where two launches give the same bits
      head_softmax_kernel        bwd 1: training; bwd 0: test_head_eval, dlogits keeps the logits
      head_gemm_kernel<false, 1, T>  Kd = K in 841, 264, 4104, 400 (K % 32 != 0: 841, 264, 4104); HW 1, 4, 49
      bst on a split shape       test_head_bn_sums: returns false, part untouched
  psx_head_sums_ok               equal to the flag of every launch above; on the host in test_head_cpu.py
  psx_head_wgrad                 test_head_wgrad[sink-gscale]: fp32 / fp16 sink, gscale 1 and 1/3, (B, K, C)
    head_wgrad_small_kernel<GT>  (1, 1, 16): one class of four, 16 of 64 channels; (33, 10, 48): K % 4 = 2,
                                 C % 64; (257, 100, 512): eight channel blocks
    head_wgrad_kernel<GT>        (33, 841, 320): K % 8 = 1, two channel blocks, the second 64 wide;
                                 (2, 4104, 64): one quarter block
    fp16 overflow                a dlogits column scaled past the fp16 range: +inf, as torch's .half()

The worst error / bound ratio of every output is printed when the module ends (profiles/
head_paths.txt holds a run's figures)."""
import pytest
import torch

from psx.ops import kernels as K

from .test_bn_gpu import RATIOS, Bufs, det_mode, dname, held
from .test_head_cpu import (BF16, F16, F32, FUSED, GSCALES, NULL_CASE, REFUSED, SLOTS, SPLIT, SUMS_CASES, TABLE,
                            WGRAD_LARGE, WGRAD_SMALL, head_inputs, head_reference, head_split, head_sums_reference,
                            head_wgrad_reference, sums_inputs, wgrad_inputs)
from .test_sgd_gpu import assert_same_bits, bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
DET = pytest.mark.parametrize("det", [False, True], ids=["float", "det"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(k for k in RATIOS if k[0].startswith("head")):
        print("head_paths ratio", *key, "%.4f" % RATIOS[key])


class Launch:
    """The placed buffers of one psx_head_fwd_bwd launch and the launch itself."""

    def __init__(self, inp, pooled=True, dact=True, loss=True, correct=True, sums=False, det=False, count=0):
        self.inp, self.B_ = inp, Bufs()
        B, HW, C, nk, dtype = (inp[k] for k in ("B", "HW", "C", "K", "dtype"))
        P = self.B_
        self.act, self.w, self.bias = P.put(inp["act"]), P.put(inp["w"]), P.put(inp["bias"])
        self.labels = P.put(inp["labels"], fill=-1)
        self.pooled = P.out(B * C) if pooled else None
        self.dl = P.out(B * nk)
        self.dact = P.out(B * HW * C, dtype) if dact else None
        self.loss = P.out(B) if loss else None
        self.correct = P.put(torch.full((1,), count, dtype=torch.int32), fill=-1, inout=True) if correct else None
        self.part = self.bst = None
        if sums:
            y1, saved = sums_inputs(B, HW, C, dtype)
            scale = K.det_slot_scale() if det else 1
            self.y1, self.saved = P.put(y1), P.put(saved)
            self.part = P.put(torch.zeros(SLOTS * 2 * C * scale), inout=True)
            self.bst = K.bwd_stats_desc(self.part.view, self.act.view, self.y1.view, self.saved.view)

    def run(self, what):
        inp = self.inp
        v = lambda p: p.view if p is not None else None
        flag = K.head_fwd_bwd(self.act.view, inp["B"], inp["HW"], inp["C"], self.w.view, self.bias.view, inp["K"],
                              self.labels.view, v(self.pooled), self.dl.view, v(self.dact), v(self.loss),
                              v(self.correct), bst=self.bst)
        self.B_.check(what)
        return flag


def _path(inp, bufs=True):
    return "split" if head_split(inp["C"], inp["K"], bufs) else "fused"


def hold(x, ref, bound, key, what):
    """held, on the flattened tensors (its report indexes the worst element)."""
    held(x.reshape(-1), ref.reshape(-1), bound.reshape(-1), key, what)


def _held(L, ref, bound, names, tag, what):
    for name in names:
        x = dict(pooled=L.pooled, loss=L.loss, dlogits=L.dl, dact=L.dact, logits=L.dl)[name]
        hold(x.view.float(), ref[name], bound[name], ("head " + name, tag), what)


@DET
@pytest.mark.parametrize("kind", ["plain", "wide", "tie", "edge_labels"])
@DT
def test_head_forward_backward(dtype, kind, det):
    with det_mode(det):
        for shape in TABLE:
            inp = head_inputs(*shape, dtype, kind)
            ref, bound = head_reference(inp)
            path = _path(inp)
            tag = "%s %s%s" % (dname(dtype), path, " det" if det else "")
            what = shape + (kind, det)
            first = Launch(inp, sums=True, det=det)
            flag = first.run(what)
            assert flag == K.head_sums_ok(inp["C"], inp["K"]) == (path == "fused"), what
            if not flag:
                assert not bool(first.part.view.any()), ("part written without the flag",) + what
            _held(first, ref, bound, ("pooled", "loss", "dlogits", "dact"), tag, what)
            assert int(first.correct.view[0]) == ref["correct"], what
            # the counter accumulates; no bst: no flag
            second = Launch(inp, count=ref["correct"])
            assert second.run(what) is False
            _held(second, ref, bound, ("pooled", "loss", "dlogits", "dact"), tag, what)
            assert int(second.correct.view[0]) == 2 * ref["correct"], what
            if det or path == "fused":  # one add per logit: the same bits every launch
                assert_same_bits(first.dl.view, second.dl.view, ("dlogits, two launches",) + what)
                assert_same_bits(first.dact.view, second.dact.view, ("dact, two launches",) + what)
                assert_same_bits(first.loss.view, second.loss.view, ("loss, two launches",) + what)


@DET
@DT
def test_head_eval(dtype, det):
    """dact null. Float atomics on the split path (ks > 1) may differ in the last bits between
    launches, so there the repeated outputs are held to their bounds instead of compared."""
    with det_mode(det):
        for shape in TABLE:
            inp = head_inputs(*shape, dtype, "plain")
            ref, bound = head_reference(inp)
            path = _path(inp)
            tag = "%s %s eval%s" % (dname(dtype), path, " det" if det else "")
            what = shape + (det,)
            same = det or path == "fused"
            names = ("pooled", "loss") + (("logits",) if path == "split" else ())
            full = Launch(inp, dact=False, sums=True, det=det)
            assert full.run(what) is False  # bst needs dact
            assert not bool(full.part.view.any()), what
            _held(full, ref, bound, names, tag, what)
            assert int(full.correct.view[0]) == ref["correct"], what
            if path == "fused":
                assert bool(torch.isnan(full.dl.view).all()), ("dlogits written in eval",) + what
            for drop in ("loss", "correct"):
                L = Launch(inp, dact=False, loss=drop != "loss", correct=drop != "correct")
                assert L.run(what) is False
                assert_same_bits(L.pooled.view, full.pooled.view, (drop, "pooled") + what)
                if L.correct is not None:
                    assert int(L.correct.view[0]) == ref["correct"], (drop,) + what
                if same:
                    assert_same_bits(L.dl.view, full.dl.view, (drop, "dlogits") + what)
                    if L.loss is not None:
                        assert_same_bits(L.loss.view, full.loss.view, (drop, "loss") + what)
                else:
                    _held(L, ref, bound, ("logits",) + (("loss",) if L.loss is not None else ()), tag, (drop,) + what)


@DT
def test_head_null_buffers_take_the_fused_kernel(dtype):
    """K C > 2^18, but without pooled the dispatcher must run the fused kernel: the BN sums are
    produced (the flag), which only it does, and everything is inside the fused bounds."""
    inp = head_inputs(*NULL_CASE, dtype, "plain")
    assert head_split(inp["C"], inp["K"]) and _path(inp, bufs=False) == "fused"
    ref, bound = head_reference(inp)
    L = Launch(inp, pooled=False, sums=True)
    assert L.run(NULL_CASE) is True
    _held(L, ref, bound, ("loss", "dlogits", "dact"), dname(dtype) + " fused", NULL_CASE)
    assert int(L.correct.view[0]) == ref["correct"]
    rows, rb = head_sums_reference(L.dact.view.cpu(), inp["act"], *sums_inputs(*NULL_CASE[:3], dtype))
    hold(L.part.view, rows, rb, ("head bn sums", dname(dtype)), NULL_CASE)


@DET
@DT
def test_head_bn_sums(dtype, det):
    key = ("head bn sums", dname(dtype) + (" det" if det else ""))
    with det_mode(det):
        for shape in SUMS_CASES:
            B, HW, C, nk = shape
            inp = head_inputs(*shape, dtype, "plain")
            ref, bound = head_reference(inp)
            y1, saved = sums_inputs(B, HW, C, dtype)
            what = shape + (det,)
            words = []
            for launch in range(2 if det else 1):
                L = Launch(inp, sums=True, det=det)
                assert L.run(what) is True
                words.append(bits(L.part.view).cpu().clone())
            if det:
                assert torch.equal(words[0], words[1]), ("two launches, different words",) + what
                rows = K.det_slot_values(L.part.view.cpu(), (SLOTS, 2, C))
            else:
                rows = L.part.view.cpu().double().view(SLOTS, 2, C)
            _held(L, ref, bound, ("dact",), dname(dtype) + " fused" + (" det" if det else ""), what)
            want, rb = head_sums_reference(L.dact.view.cpu(), inp["act"], y1, saved)  # dact as stored
            hold(rows, want, rb, key, what)
            if B < SLOTS:
                assert not bool(rows[B:].any()), ("a row without samples was written",) + what
            # no dact: no sums, part untouched (it is checked as an input)
            E_ = Launch(inp, dact=False, det=det)
            P = E_.B_
            E_.y1, E_.saved = P.put(y1), P.put(saved)
            E_.part = P.put(torch.zeros(SLOTS * 2 * C * (K.det_slot_scale() if det else 1)))
            E_.bst = K.bwd_stats_desc(E_.part.view, E_.act.view, E_.y1.view, E_.saved.view)
            assert E_.run(what) is False
        # a split-path shape: no sums
        inp = head_inputs(*SPLIT[0], dtype, "plain")
        S = Launch(inp, det=det)
        P = S.B_
        y1, saved = sums_inputs(*SPLIT[0][:3], dtype)
        S.y1, S.saved = P.put(y1), P.put(saved)
        S.part = P.put(torch.zeros(SLOTS * 2 * inp["C"] * (K.det_slot_scale() if det else 1)))
        S.bst = K.bwd_stats_desc(S.part.view, S.act.view, S.y1.view, S.saved.view)
        assert S.run(SPLIT[0]) is False


@pytest.mark.parametrize("gscale", GSCALES, ids=["g1", "g1/3"])
@pytest.mark.parametrize("sink", [F32, F16], ids=["fp32", "fp16"])
def test_head_wgrad(sink, gscale):
    for shape in WGRAD_SMALL + WGRAD_LARGE:
        B, nk, C = shape
        kern = "small" if shape in WGRAD_SMALL else "large"
        for overflow in (False, True) if sink == F16 else (False,):
            dl, pooled = wgrad_inputs(B, nk, C, overflow)
            P = Bufs()
            d, p = P.put(dl), P.put(pooled)
            dw, db = P.out(nk * C, sink), P.out(nk, sink)
            K.head_wgrad(d.view, p.view, B, nk, C, dw.view.data_ptr(), db.view.data_ptr(), gscale, sink == F16)
            what = shape + (gscale, overflow)
            P.check(what)
            rw, rb, b_dw, b_db = head_wgrad_reference(dl, pooled, gscale, sink)
            gw, gb = dw.view.cpu().view(nk, C), db.view.cpu()
            lo = 1 if overflow else 0
            if overflow:  # past 65504 by half again and more: +inf, as torch's conversion of the fp32 value gives
                assert float(rw[0].min()) > 1e5 and float(rb[0]) > 1e5
                assert torch.equal(gw[0], rw[0].float().half()) and bool(torch.isinf(gw[0]).all()), what
                assert torch.equal(gb[:1], rb[:1].float().half()) and bool(torch.isinf(gb[:1]).all()), what
            key = dname(sink) + " " + kern
            if nk > lo:
                hold(gw[lo:].float(), rw[lo:], b_dw[lo:], ("head dw", key), what)
                hold(gb[lo:].float(), rb[lo:], b_db[lo:], ("head db", key), what)


@DT
def test_head_refusals(dtype):
    """-2 before any launch: the call raises and every output keeps its NaN."""
    for C, nk in REFUSED:
        B, HW = 2, 1
        gen = torch.Generator().manual_seed(C + nk)
        inp = dict(B=B, HW=HW, C=C, K=nk, dtype=dtype, act=torch.rand(B, HW, C, generator=gen).to(dtype),
                   w=torch.randn(nk, C, generator=gen), bias=torch.zeros(nk),
                   labels=torch.zeros(B, dtype=torch.int32))
        assert not K.head_sums_ok(C, nk)
        for dact in (True, False):
            L = Launch(inp, dact=dact, sums=True)
            with pytest.raises(RuntimeError):
                L.run((C, nk))
            L.B_.check((C, nk, dact))
            for out in (L.pooled, L.dl, L.dact, L.loss):
                assert out is None or bool(torch.isnan(out.view).all()), (C, nk, dact)
            assert int(L.correct.view[0]) == 0 and not bool(L.part.view.any()), (C, nk, dact)
