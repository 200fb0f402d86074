"""The weight-gradient kernels (csrc/kernels/wgrad_v2.hip, the stem's in stem.hip) and their split-K
reduction (csrc/kernels/wgrad_reduce.hip), directly, on every route the planner takes, bit for bit
against the fp64 references of tests/test_wgrad_cpu.py (exact integer operands: no tolerance), plus
one random-operand case per family and dtype inside the per-element bound stated there.

Every launch (launch): K.conv_wgrad2_path must first report the route the case names; operands and
partials lie between canaries, the partials pre-filled with NaN; the returned split count is the
query's; EVERY SLAB equals its own reference (not only their sum: two split-boundary mistakes cancel
in the sum), the padding columns are 0 and nothing is NaN. The stem's 256 slabs (tile t of 4 output
rows goes to slab t % 256, columns below 196 written) are compared one by one and as their sum.
Then the launch's partials are reduced by K.wgrad_reduce into a gradient between NaN guard zones,
on the fp32 and the fp16 wire, at scale 1 and 2^-7, each from a fresh copy (the pre-sum consumes its
partials): equal to the reference, the guard zones still NaN.

  wgrad2_kernel / wgrad2f_kernel, every tile      test_exact[tile*], the edge cases (H != W, stride 2
                                                  on an odd image, 1x1 stride 2, the ident path, 7x7 /
                                                  s2 / p3 with cin 3, cp 8 / 4 with a padded Kg, fewer
                                                  pixels than a step, one more than a step)
  wgrad3_kernel, both width kinds, NS 3 / 6,      test_exact[tap*-bf16, gen*-bf16], H != W: 4x8, 8x2,
  BC 64 / 128 (NS 3)                              3x7, 4x14, 7x8, 7x2
  wgrad3f_kernel, BC 64 / 128                     test_exact[tap*-f32]
  stem7_wgrad_kernel                              test_exact[stem7-n1-f32, stem7-n3-f32]
  the four fp32 tile kernels as 1x1 TN GEMMs      test_bgemm_tn_f32_tiles (128x128 is reached no other
                                                  way)
  wgrad_reduce2_kernel, wgrad_reduce_kernel,      test_reduce_alone on synthetic integer slabs with NaN
  wgrad_presum_kernel                             wherever the reduction must not look (the cases and
                                                  what each is for: test_wgrad_cpu.reduce_cases)
  wgrad_reduce2_batch_kernel                      test_reduce_batch: 1 to 4 mixed layers against fp64
  accuracy class                                  test_numerics (ratios printed)
  refusals                                        test_wgrad_refusals, test_reduce_refusals: the code,
                                                  the query's answer, partials and output untouched
"""
import ctypes as C
import math

import pytest
import torch

from psx.ops import kernels as K
from psx.ops._lib import HipError, kernels, ptr, stream_ptr

from .test_sgd_cpu import assert_within
from .test_sgd_gpu import DEV, Placed, assert_same_bits
from .test_wgrad_cpu import (ALL_EXACT, BATCHES, F16, F32, NAN, NUMERICS, REDUCE_CASES, SCALES, ids, numerics_reference,
                             operands, presum_applies, query_route, reduce_reference, reduce_slabs, ref_oihw, ref_slabs)

pytestmark = pytest.mark.gpu


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault: nothing more may run on this device
        pytest.exit(f"GPU fault in {what}: {e}", returncode=3)


class Guarded:
    """``n`` elements of NaN between two guard zones of NaN that a launch must leave as they are."""
    ZONE = 256

    def __init__(self, n, dtype):
        self.big = torch.full((n + 2 * self.ZONE,), NAN, dtype=dtype, device=DEV)
        self.view = self.big[self.ZONE:self.ZONE + n]

    def guards_intact(self):
        return bool(torch.isnan(self.big[:self.ZONE]).all()) and bool(torch.isnan(self.big[-self.ZONE:]).all())

    def untouched(self):
        return bool(torch.isnan(self.big).all())


def check_reduce(part_values, want, splits, oc, kg, cin, ic, k, what):
    """K.wgrad_reduce of the partials ``part_values`` (fp32, flat) on both wires at both scales, each
    from a fresh copy; ``want(scale, fp16)``: the reference in the wire's dtype."""
    for fp16 in (False, True):
        for scale in SCALES:
            part = Placed(part_values)
            out = Guarded(oc * cin * k * k, F16 if fp16 else F32)
            K.wgrad_reduce(part.view, splits, oc, kg, cin, ic, k, scale, out.view.data_ptr(), fp16)
            _sync(what)
            assert part.intact() and out.guards_intact(), (what, "wrote outside its buffers")
            assert_same_bits(out.view, want(scale, fp16).reshape(-1), (what, "fp16" if fp16 else "fp32", scale))
            if not presum_applies(splits, oc, kg, ic, k):
                assert part.unchanged(), (what, "partials changed without a pre-sum")


def launch(case, numerics=False):
    """The weight gradient of the case along its asserted route: (path, partials [splits][OC][Kg] on
    the host, fp32)."""
    path = query_route(case)
    _, _, xp, dyf = operands(case, numerics)
    x, dy = Placed(xp.to(case.dtype).reshape(-1)), Placed(dyf.to(case.dtype).reshape(-1))
    part = Placed(torch.full((path["splits"] * case.oc * case.kg,), NAN))
    ns = K.conv_wgrad2(x.view, dy.view, part.view, *case.args()[:-1])
    _sync(case.id)
    assert ns == path["splits"], (case.id, "split count", ns, path)
    assert x.intact() and dy.intact() and part.intact(), (case.id, "canary overwritten")
    assert x.unchanged() and dy.unchanged(), (case.id, "operand changed")
    return path, part.view.cpu().view(path["splits"], case.oc, case.kg)


@pytest.mark.parametrize("case", ALL_EXACT, ids=ids(ALL_EXACT))
def test_exact(case):
    path, got = launch(case)
    ref = ref_slabs(case, path)
    cols = case.k ** 2 * case.cp
    if path["kind"] == "stem7":  # its columns >= 196 are not written
        got_w = got[:, :, :cols]
        assert torch.equal(got_w.double().sum(0), ref.sum(0)[:, :cols]), (case.id, "sum of the slabs")
        ref = ref[:, :, :cols]
    else:
        got_w = got
        assert not bool(got[:, :, cols:].any()), (case.id, "padding columns not zero")
    assert not bool(torch.isnan(got_w).any()), (case.id, "NaN left in the partials")
    for s in range(path["splits"]):
        ne = got_w[s].double() != ref[s]
        assert not bool(ne.any()), (case.id, "slab", s, "of", path["splits"], "elements that differ", int(ne.sum()),
                                    "first (oc, column)", ne.nonzero()[0].tolist())
    check_reduce(got.reshape(-1), lambda scale, fp16: ref_oihw(case, path, scale, fp16), path["splits"], case.oc,
                 case.kg, case.ci, case.cp, case.k, case.id)


@pytest.mark.parametrize("case", NUMERICS, ids=ids(NUMERICS))
def test_numerics(case):
    """Random bf16-representable operands: every element of the reduced gradient inside its bound."""
    path, got = launch(case, numerics=True)
    for fp16 in (False, True):
        for scale in SCALES:
            part = Placed(got.reshape(-1))
            out = Guarded(case.oc * case.ci * case.k ** 2, F16 if fp16 else F32)
            K.wgrad_reduce(part.view, path["splits"], case.oc, case.kg, case.ci, case.cp, case.k, scale,
                           out.view.data_ptr(), fp16)
            _sync(case.id)
            assert part.intact() and out.guards_intact()
            ref, bound = numerics_reference(case, path, scale, fp16)
            y = out.view.cpu().reshape(-1)
            ratio = float(((y.double() - ref.reshape(-1)).abs() / bound.reshape(-1).clamp_min(1e-300))
                          .nan_to_num(nan=math.inf).max())
            print("wgrad_paths numerics", case.id, "fp16" if fp16 else "fp32", scale, "%.4f" % ratio)
            assert_within(y, ref.reshape(-1), bound.reshape(-1), (case.id, fp16, scale))


@pytest.mark.parametrize("br,bc", [(64, 64), (64, 128), (128, 64), (128, 128)], ids=lambda v: str(v))
def test_bgemm_tn_f32_tiles(br, bc):
    """The four fp32 tile kernels as batched TN GEMMs, part[b q + j] = D[b, range j]^T X[b, range j]:
    q splits of 1, 5 and 11 (one split) 32-pixel steps, exact integer operands, NaN-filled slabs."""
    nb, Cc, Kc = 2, 128, 128
    gen = torch.Generator().manual_seed(br + bc)
    for q, T in ((5, 160), (2, 320), (1, 352)):
        X = torch.randint(-3, 4, (nb, T, Cc), generator=gen).double()
        D = torch.randint(-2, 3, (nb, T, Kc), generator=gen).double()
        r = T // q
        ref = torch.stack([D[b, j * r:(j + 1) * r].t() @ X[b, j * r:(j + 1) * r] for b in range(nb) for j in range(q)])
        x, d = Placed(X.float().reshape(-1)), Placed(D.float().reshape(-1))
        part = Placed(torch.full((nb * q * Kc * Cc,), NAN))
        K.bgemm_tn_f32(x.view, d.view, part.view, T, Cc, Kc, nb, q, br, bc)
        _sync(("bgemm_tn", br, bc, q))
        assert x.intact() and d.intact() and part.intact() and x.unchanged() and d.unchanged()
        assert torch.equal(part.view.cpu().double(), ref.reshape(-1)), ("bgemm_tn", br, bc, q, T)


@pytest.mark.parametrize("rc", REDUCE_CASES, ids=ids(REDUCE_CASES))
def test_reduce_alone(rc):
    s = reduce_slabs(rc)
    check_reduce(s.float().reshape(-1), lambda scale, fp16: reduce_reference(s, rc.cin, rc.ic, rc.k, scale, fp16),
                 rc.splits, rc.oc, rc.kg, rc.cin, rc.ic, rc.k, rc.id)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("layers", BATCHES, ids=[f"n{len(b)}" for b in BATCHES])
def test_reduce_batch(layers, fp16):
    """wgrad_reduce_batch of 1 to 4 mixed layers (1x1 / 3x3 / 5x5 / 7x7, padded channels, IC 96, one
    to 57 splits) against fp64, every layer's output between NaN guard zones."""
    scale = SCALES[1]
    parts = [Placed(reduce_slabs(rc).float().reshape(-1)) for rc in layers]
    outs = [Guarded(rc.oc * rc.cin * rc.k ** 2, F16 if fp16 else F32) for rc in layers]
    K.wgrad_reduce_batch([(p.view, rc.splits, rc.oc, rc.kg, rc.cin, rc.ic, rc.k, o.view.data_ptr())
                          for rc, p, o in zip(layers, parts, outs)], scale, fp16)
    _sync("reduce_batch")
    for rc, p, o in zip(layers, parts, outs):
        assert p.intact() and p.unchanged() and o.guards_intact(), rc.id
        want = reduce_reference(reduce_slabs(rc), rc.cin, rc.ic, rc.k, scale, fp16)
        assert_same_bits(o.view, want.reshape(-1), ("batch", len(layers), rc.id))


def _code(fn, *a, **kw):
    with pytest.raises(HipError) as e:
        fn(*a, **kw)
    return int(str(e.value).rsplit(" ", 1)[1])


REFUSED = [  # (n, h, w, ic, oc, k, stride, pad, kg, f32)
    (2, 4, 4, 64, 96, 3, 1, 1, 576, False),    # OC % 64
    (2, 4, 4, 64, 64, 3, 1, 1, 600, False),    # Kg % 64
    (2, 4, 4, 48, 64, 3, 1, 1, 448, False),    # tile route, IC no power of two
    (2, 4, 4, 48, 64, 3, 1, 1, 448, True),
    (2, 4, 4, 48, 64, 1, 1, 0, 64, False),
    (2, 4, 4, 48, 64, 1, 1, 0, 64, True),
    (2, 4, 4, 4, 64, 3, 1, 1, 64, False),      # bf16: less than one 16-byte chunk of channels
    (2, 5, 7, 192, 64, 3, 1, 1, 1728, False),  # IC 192 off the tap-reuse routes
    (2, 5, 7, 192, 64, 3, 1, 1, 1728, True),
]


@pytest.mark.parametrize("g", REFUSED, ids=lambda g: "-".join(map(str, g)))
def test_wgrad_refusals(g):
    """A geometry route_wgrad refuses: the query answers -2, the launch raises with -2 and leaves
    the partials untouched."""
    n, h, w, ic, oc, k, stride, pad, kg, f32 = g
    assert K.conv_wgrad2_path(*g) == -2
    T = F32 if f32 else torch.bfloat16
    oh, ow = K.conv_out_hw(h, w, k, stride, pad)
    x, dy = Placed(torch.ones(n * h * w * ic, dtype=T)), Placed(torch.ones(n * oh * ow * oc, dtype=T))
    part = Guarded(4 * oc * kg, F32)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        K.conv_wgrad2(x.view, dy.view, part.view, n, h, w, ic, oc, k, stride, pad, kg)
    _sync("refusal")
    assert part.untouched() and x.intact() and dy.intact()


def _batch_raw(n, items, scale, fp16):
    """psx_wgrad_reduce_batch with ``n`` as given (K.wgrad_reduce_batch asserts 1 <= n <= 4)."""
    m = len(items)
    P = (C.c_void_p * m)(*[ptr(it[0]) for it in items])
    O = (C.c_void_p * m)(*[it[7] for it in items])
    col = [(C.c_int * m)(*[int(it[j]) for it in items]) for j in (1, 2, 3, 4, 5)]
    rs = (C.c_int * m)(*[int(it[6]) ** 2 for it in items])
    return int(kernels().psx_wgrad_reduce_batch(n, P, O, *col, rs, float(scale), int(fp16), stream_ptr()))


def test_reduce_refusals():
    """psx_wgrad_reduce: -2 where the one-thread-per-column kernel's OC Kg is no multiple of 256.
    psx_wgrad_reduce_batch: -2 for no layer or more than four, -3 for a layer the v2 kernel does not
    take (R S > 49, IC % 16). Nothing is launched: the output stays NaN, the partials as they were."""
    part = Placed(torch.ones(4 * 64 * 1344))
    out = Guarded(64 * 64 * 81, F32)
    o = out.view.data_ptr()
    assert _code(K.wgrad_reduce, part.view, 2, 3, 128, 5, 8, 3, 1.0, o, False) == -2   # 3 x 128 columns
    assert _code(K.wgrad_reduce, part.view, 2, 5, 1344, 16, 16, 9, 1.0, o, True) == -2
    good = (part.view, 2, 64, 576, 64, 64, 3, o)
    assert _batch_raw(0, [good], 1.0, False) == -2
    assert _batch_raw(5, [good] * 5, 1.0, False) == -2
    assert _code(K.wgrad_reduce_batch, [good, (part.view, 2, 64, 1344, 16, 16, 9, o)], 1.0, False) == -3
    assert _code(K.wgrad_reduce_batch, [(part.view, 2, 64, 128, 5, 8, 3, o), good], 1.0, True) == -3
    assert not K.wgrad_reduce_batchable(16, 9) and not K.wgrad_reduce_batchable(8, 3) and K.wgrad_reduce_batchable(96, 7)
    _sync("reduce refusals")
    assert out.untouched() and part.intact() and part.unchanged()
