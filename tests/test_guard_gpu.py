"""The gradient-guard kernels (csrc/kernels/gguard.hip) against sgd_apply_multi and fp64: the
unclipped update is sgd_apply_multi's bit for bit, the norm and the clipping coefficient are
within bounds derived from the accumulation (below), the clipped update is sgd_apply_multi's with
the coefficient read back, non-finite rounds leave everything untouched, both entries and repeated
runs agree in every bit, canaries survive, the launches replay from a HIP graph, and bad arguments
are refused before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from psx.ops import kernels as K
from psx.ops._lib import kernels as klib
from psx.ops._lib import ptr, stream_ptr

pytestmark = pytest.mark.gpu

DEV = "cuda"
CH = K.GUARD_CHUNK
E = CH // 256        # elements one lane accumulates in fp32 before the reduction goes to double
U = 2.0 ** -24
# the norm: each fma adds at most 2^-24 relative error to a non-negative sum (E of them), the
# conversion of gscale and the double steps are far below one more, the square root halves the
# total, the comparison's own fp64 reference and the state's stores add the rest: (E + 2) * 2^-24
NORM_RTOL = (E + 2) * U
COEF_RTOL = (E + 3) * U  # the division and the rounding to float on top
LR = 0.1
NS = [5, 8, CH, CH + 1, 3 * CH + 5, 100003]
NMAX = max(NS)
WS = [1, 2, 7, 32]
PADS = {"aligned": 8, "offset": 9}  # elements in front of every base pointer: 9 = the scalar path
MOMS = [dict(momentum=0.0, first=False), dict(momentum=0.9, first=True), dict(momentum=0.9, first=False)]


def _case(ni, align, wi):
    """Every n x alignment x W; the other axes rotate so that each value of each meets every
    (n, alignment): wire dtype and weight decay over W's index, momentum form and image with n."""
    return dict(n=NS[ni], pad=PADS[align], W=WS[wi], dtype=(torch.float16, torch.float32)[wi % 2],
                wd=(0.0, 5e-4)[(wi // 2) % 2], img_on=bool((wi + ni) % 2), **MOMS[(wi + ni) % 3])


CASES = [pytest.param(_case(ni, al, wi), id=f"n{NS[ni]}-{al}-W{WS[wi]}")
         for ni in range(len(NS)) for al in PADS for wi in range(len(WS))]
SOME = [pytest.param(_case(ni, al, (ni + k) % 4), id=f"n{NS[ni]}-{al}")
        for ni in range(len(NS)) for k, al in enumerate(PADS)]


@pytest.fixture(scope="module")
def data():
    """CPU inputs, built once: weights, momentum buffer, 32 gradients."""
    gen = torch.Generator().manual_seed(1234)
    p = torch.randn(NMAX, generator=gen) * 0.05
    v = torch.randn(NMAX, generator=gen) * 1e-2
    gs = [torch.randn(NMAX, generator=gen) * 1e-2 for _ in range(32)]
    return p, v, gs


def _banded(x, pad, fill):
    """x on the device inside an allocation with ``pad`` canary elements on either side."""
    big = torch.full((pad + x.numel() + pad,), fill, dtype=x.dtype, device=DEV)
    big[pad:pad + x.numel()] = x.to(DEV)
    return big, big[pad:pad + x.numel()]


def _intact(big, pad, fill):
    ref = torch.full((pad,), fill, dtype=big.dtype, device=DEV)
    return torch.equal(big[:pad], ref) and torch.equal(big[-pad:], ref)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _state(n, pad=8):
    """A GuardState whose partials sit between canaries."""
    st = K.GuardState(n, DEV)
    st.partials_big, st.partials = _banded(torch.zeros(st.nblocks, dtype=torch.float64), pad, -3.0)
    return st


class Bufs:
    """Device buffers of one case between canaries; the sources are passed in (CPU tensors)."""

    def __init__(self, data, c, srcs=None):
        p, v, gs = data
        n, pad = c["n"], c["pad"]
        self.c, self.n, self.pad = c, n, pad
        self.big = {"p": _banded(p[:n], pad, 7.0), "stage": _banded(torch.zeros(n), pad, 9.0)}
        if c["momentum"]:
            self.big["buf"] = _banded(v[:n], pad, 5.0)
        if c["img_on"]:
            self.big["img"] = _banded(torch.zeros(n, dtype=torch.bfloat16), pad, 3.0)
        srcs = [g[:n].to(c["dtype"]) for g in gs[: c["W"]]] if srcs is None else srcs
        self.src_big = [_banded(s, pad, 1.0) for s in srcs]
        self.srcs = [b[1] for b in self.src_big]
        self.gscale = 1.0 / len(srcs)

    def __getattr__(self, k):  # p, stage, buf, img: the view between the canaries, None when off
        if k not in ("p", "stage", "buf", "img"):
            raise AttributeError(k)
        return self.big[k][1] if k in self.big else None

    def hp(self, gscale=None):
        c = self.c
        return dict(lr=LR, gscale=self.gscale if gscale is None else gscale, momentum=c["momentum"], wd=c["wd"],
                    buf=self.buf, first=c["first"], n=self.n, img=self.img)

    def sgd(self, gscale=None):
        K.sgd_apply_multi(self.p, self.srcs, **self.hp(gscale))

    def guard(self, st, clip, dense=False):
        if dense:
            K.guard_apply(self.p, self.stage, st, clip_norm=clip, **self.hp())
        else:
            K.guard_apply_multi(self.p, self.srcs, self.stage, st, clip_norm=clip, **self.hp())

    def outs(self):
        return {k: v[0].clone() for k, v in self.big.items() if k != "stage"}

    def canaries(self):
        fills = {"p": 7.0, "stage": 9.0, "buf": 5.0, "img": 3.0}
        return all(_intact(v[0], self.pad, fills[k]) for k, v in self.big.items()) and \
            all(_intact(b[0], self.pad, 1.0) for b in self.src_big)


def _same(a: dict, b: dict):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _torch_sum(srcs):
    """s in fp32 in source order from 0.f, and sqrt(sum s^2) in fp64 over that s."""
    s = torch.zeros(srcs[0].numel(), dtype=torch.float32, device=DEV)
    for g in srcs:
        s = s + g.float()
    return s, float(s.double().square().sum().sqrt())


# ---------------------------------------------------------------------------- no clipping, norm, staging
@pytest.mark.parametrize("c", CASES)
def test_unclipped_is_sgd_apply_multi(data, c):
    ref = Bufs(data, c)
    ref.sgd()
    want = ref.outs()
    s, root = _torch_sum(ref.srcs)
    norm64 = float(np.float32(ref.gscale)) * root
    for clip in (0.0, 1e30):
        b, st = Bufs(data, c), _state(c["n"])
        b.guard(st, clip)
        assert _same(b.outs(), want), clip
        assert torch.equal(b.stage.view(torch.int32), s.view(torch.int32))  # the staged sum, bit for bit
        r = st.read()
        assert r["coef"] == 1.0 and r["skip"] is False
        assert (r["rounds"], r["clipped_rounds"], r["skipped_rounds"]) == (1, 0, 0)
        rel = abs(r["norm"] - norm64) / norm64
        print(f"norm rel err {rel / U:.2f} x 2^-24 (bound {E + 2})")
        assert rel <= NORM_RTOL
        assert r["norm_last"] == r["norm"] == r["norm_max"] == r["norm_sum"]
        assert abs(r["S"] - root * root) <= 2 * NORM_RTOL * root * root
        assert b.canaries() and _intact(st.partials_big, 8, -3.0)


# ---------------------------------------------------------------------------- clipping
@pytest.mark.parametrize("c", CASES)
def test_clipped_is_sgd_apply_multi_scaled(data, c):
    b, st = Bufs(data, c), _state(c["n"])
    _, root = _torch_sum(b.srcs)
    norm64 = float(np.float32(b.gscale)) * root
    clip = float(np.float32(0.25 * norm64))
    b.guard(st, clip)
    r = st.read()
    want_coef = clip / (norm64 + 1e-6)
    rel = abs(r["coef"] - want_coef) / want_coef
    print(f"coef rel err {rel / U:.2f} x 2^-24 (bound {E + 3})")
    assert rel <= COEF_RTOL and 0.2 < r["coef"] < 0.3
    assert (r["rounds"], r["clipped_rounds"], r["skipped_rounds"]) == (1, 1, 0) and r["skip"] is False
    ref = Bufs(data, c)  # the parent's kernel with the coefficient (checked above) folded into gscale
    ref.sgd(float(np.float32(b.gscale) * np.float32(r["coef"])))
    assert _same(b.outs(), ref.outs())
    plain = Bufs(data, c)
    plain.sgd()
    assert not torch.equal(plain.p, b.p)
    assert b.canaries() and _intact(st.partials_big, 8, -3.0)


# ---------------------------------------------------------------------------- dense entry, determinism
@pytest.mark.parametrize("c", SOME)
def test_dense_entry_and_reruns_give_the_same_bits(data, c):
    probe = Bufs(data, c)
    clip = float(np.float32(0.5 * np.float32(probe.gscale) * _torch_sum(probe.srcs)[1]))  # half the norm: clips
    runs = []
    for dense in (False, False, True):
        b, st = Bufs(data, c), _state(c["n"])
        if dense:
            b.stage.copy_(_torch_sum(b.srcs)[0])
        b.guard(st, clip, dense=dense)
        assert st.read()["clipped_rounds"] == 1
        runs.append((b.outs(), st.state.clone(), st.partials.clone(), b.stage.clone()))
        assert b.canaries() and _intact(st.partials_big, 8, -3.0)
    for other in runs[1:]:
        assert _same(other[0], runs[0][0])
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(other[1:], runs[0][1:]))


# ---------------------------------------------------------------------------- skipped rounds
N_SKIP = 3 * CH + 5
SKIP_AT = {"head": 0, "body": CH + 8 * 300 + 3, "tail": N_SKIP - 4, "last": N_SKIP - 1}


@pytest.mark.parametrize("align", list(PADS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("where,value", [("head", "inf"), ("body", "-inf"), ("tail", "nan"), ("last", "inf"),
                                         ("body", "nan"), ("head", "+-inf")])
def test_nonfinite_round_is_skipped(data, where, value, dtype, align):
    c = dict(n=N_SKIP, pad=PADS[align], W=2, dtype=dtype, wd=5e-4, img_on=True, momentum=0.9, first=False)
    good = [g[:N_SKIP].to(dtype) for g in data[2][:2]]
    bad = [g.clone() for g in good]
    i = SKIP_AT[where]
    if value == "+-inf":  # finite everywhere in fp32 except where the two meet: inf - inf
        bad[0][i], bad[1][i] = float("inf"), float("-inf")
    else:
        bad[1][i] = float(value)
    b, st = Bufs(data, c, bad), _state(N_SKIP)
    before = b.outs()
    b.guard(st, 1.0)
    r = st.read()
    assert r["skip"] is True and r["coef"] == 0.0 and not np.isfinite(r["S"])
    assert (r["rounds"], r["clipped_rounds"], r["skipped_rounds"]) == (1, 0, 1)
    assert r["norm_max"] == 0.0 and r["norm_sum"] == 0.0
    assert _same(b.outs(), before) and b.canaries()
    # the next, finite round on the same buffers and state: the bits of a fresh run
    for dst, g in zip(b.srcs, good):
        dst.copy_(g)
    b.guard(st, 0.0)
    fresh, fst = Bufs(data, c, good), _state(N_SKIP)
    fresh.guard(fst, 0.0)
    assert _same(b.outs(), fresh.outs())
    r, f = st.read(), fst.read()
    assert (r["rounds"], r["clipped_rounds"], r["skipped_rounds"]) == (2, 0, 1) and r["skip"] is False
    assert r["norm"] == f["norm"] == r["norm_max"] == r["norm_sum"]


def test_32_sources_of_fp16_max_stay_finite(data):
    """32 x 65504 at one index: 2096128 in fp32, its square 4.4e12: applied, not skipped."""
    c = dict(n=CH + 1, pad=8, W=32, dtype=torch.float16, wd=0.0, img_on=True, momentum=0.0, first=False)
    srcs = [g[: c["n"]].half() for g in data[2][:32]]
    for s in srcs:
        s[CH - 3] = 65504.0
    b, st = Bufs(data, c, srcs), _state(c["n"])
    b.guard(st, 0.0)
    r = st.read()
    assert r["skip"] is False and r["coef"] == 1.0 and r["skipped_rounds"] == 0
    assert float(b.stage[CH - 3]) == 32 * 65504.0
    ref = Bufs(data, c, srcs)
    ref.sgd()
    assert _same(b.outs(), ref.outs())


# ---------------------------------------------------------------------------- graph capture
def test_graph_replay_decides_on_the_device(data):
    """The three launches captured once; replays with the sources rewritten: an unclipped, a
    clipped and a non-finite round each equal the eager call, and the counters read 3 / 1 / 1."""
    n = CH + 1
    c = dict(n=n, pad=8, W=2, dtype=torch.float16, wd=5e-4, img_on=True, momentum=0.9, first=False)
    small = [g[:n].half() for g in data[2][:2]]
    large = [(8 * g[:n]).half() for g in data[2][2:4]]
    inf = [g.clone() for g in small]
    inf[0][n - 1] = float("inf")
    rounds = [small, large, inf]
    clip = 2.0 * 0.5 * _torch_sum([g.to(DEV) for g in small])[1]  # twice the small round's norm
    eager, est = Bufs(data, c, small), _state(n)
    cap, cst = Bufs(data, c, small), _state(n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.guard(cst, clip)
    for k, v in Bufs(data, c, small).big.items():  # a capture does not run: restore the inputs anyway
        cap.big[k][0].copy_(v[0])
    cst.state.zero_()
    for wires in rounds:
        for b in (eager, cap):
            for dst, g in zip(b.srcs, wires):
                dst.copy_(g)
        eager.guard(est, clip)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager.outs(), cap.outs())
        assert torch.equal(est.state, cst.state)
    r = cst.read()
    assert (r["rounds"], r["clipped_rounds"], r["skipped_rounds"]) == (3, 1, 1) and r["skip"] is True
    assert cap.canaries() and _intact(cst.partials_big, 8, -3.0)


# ---------------------------------------------------------------------------- argument checks
def test_argument_checks(data):
    """Every rejected argument returns hipErrorInvalidValue and launches nothing: parameters and
    the state block stay as they were."""
    n = CH + 1
    c = dict(n=n, pad=8, W=2, dtype=torch.float32, wd=0.0, img_on=False, momentum=0.0, first=False)
    b, st = Bufs(data, c), _state(n)
    before = b.outs()
    lib = klib()
    arr = (C.c_void_p * 2)(*[s.data_ptr() for s in b.srcs])
    hole = (C.c_void_p * 2)(b.srcs[0].data_ptr(), None)
    alias = (C.c_void_p * 2)(b.srcs[0].data_ptr(), b.stage.data_ptr())

    def multi(p=b.p, srcs=arr, nsrc=2, stage=b.stage, n=n, partials=st.partials, state=st.state, clip=0.0):
        return lib.psx_guard_apply_multi(ptr(p), srcs, nsrc, 0, ptr(stage), None, n, ptr(partials), ptr(state), LR, 0.5,
                                         0.0, 0.0, clip, 0, None, stream_ptr())

    def dense(p=b.p, stage=b.stage, n=n, partials=st.partials, state=st.state, clip=0.0):
        return lib.psx_guard_apply(ptr(p), ptr(stage), None, n, ptr(partials), ptr(state), LR, 0.5, 0.0, 0.0, clip, 0,
                                   None, stream_ptr())

    big = (C.c_void_p * 33)(*([b.srcs[0].data_ptr()] * 33))
    bad = [multi(nsrc=0), multi(srcs=big, nsrc=33), multi(srcs=None), multi(p=None), multi(stage=None),
           multi(partials=None), multi(state=None), multi(srcs=hole), multi(srcs=alias), multi(n=0), multi(n=-5),
           multi(clip=-1.0), multi(clip=float("nan")),
           dense(p=None), dense(stage=None), dense(partials=None), dense(state=None), dense(n=0), dense(clip=-0.5)]
    assert bad == [1] * len(bad), bad  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert _same(b.outs(), before) and st.read()["rounds"] == 0
    assert torch.equal(b.stage, torch.zeros(n, device=DEV))
    assert multi() == 0 and dense() == 0  # the same calls with good arguments run
    assert st.read()["rounds"] == 2
    with pytest.raises(AssertionError):
        K.guard_apply_multi(b.p, b.srcs, b.stage, st, LR, clip_norm=-1.0, n=n)
    with pytest.raises(AssertionError):
        K.guard_apply_multi(b.p, [b.srcs[0], b.stage], b.stage, st, LR, n=n)
