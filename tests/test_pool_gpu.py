"""The max-pool kernels of csrc/kernels/pool.hip, directly, against the reference of
tests/test_pool_cpu.py, on inputs where ties are the rule. Every buffer lies among canaries;
outputs are pre-filled (NaN, and 255 for the tap index, which no window has), inputs are checked
unchanged. y and arg must match bit for bit; dx must equal the reference's fp32 sum in the kernel's
(doh, dow) order bit for bit (for bf16: its bf16 rounding), which is the float64 sum exactly where
at most one window selects the pixel and within one fp32 add's rounding per further window
(tests/test_pool_cpu.py::test_dx32_is_the_sum_within_its_roundings), and +0 where none does.
Shapes are (B, H, W, C).

Which test reaches which branch:

  psx_maxpool3s2_fwd              test_maxpool[dtype-kind]
    maxpool3s2_fwd_kernel<T>      T = float / uint16_t; C 8 (one vector per pixel), 16, 64; (1, 1, 1, 8): one
                                  output, eight of nine taps in the padding; (2, 2, 1, 8): H 2, W 1; (3, 7, 9,
                                  16): odd sizes, OH 4, OW 5; (2, 16, 16, 64): even sizes, 4 workgroups
      f > best (strict)           kinds relu_bf16 and constant: the first tap inside the image wins
      padding skipped             kind negative: reading the padding as 0 would win every border window
      second grid-stride trip     test_maxpool_past_the_grid_cap: (3, 224, 224, 512) bf16, 2,408,448 threads'
                                  worth of work on 8192 x 256
    C % 8: -2                     test_maxpool_refuses_c12 (and, with the 2^31 refusal, on the host in
                                  tests/test_pool_cpu.py)
  psx_maxpool3s2_bwd              the same tests
    maxpool3s2_bwd_kernel<T>      blocks cut by the image (ih >= H, iw >= W: H, W of 1, 7, 9), windows cut
                                  (oh >= OH, ow >= OW: every shape's last block row / column); pixels no window
                                  selects are written as 0 (the pre-fill is NaN); up to four windows select
                                  one pixel in kind constant

The worst |dx - float64 sum| over its rounding allowance is printed when the module ends
(profiles/pool_paths.txt holds a run's figures)."""
import pytest
import torch

from psx.ops import kernels as K

from .test_bn_gpu import RATIOS, Bufs, dname
from .test_pool_cpu import BF16, F32, GRID_CAP_SHAPE, KINDS, SHAPES, U, maxpool_reference, out_hw, pool_inputs
from .test_sgd_gpu import DEV, assert_same_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
DT = pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(k for k in RATIOS if k[0].startswith("pool")):
        print("pool_paths ratio", *key, "%.4f" % RATIOS[key])


def _run(x, dy, what):
    """Forward and backward on placed buffers: (y, arg, dx) views, after the canary checks."""
    B, H, W, C = x.shape
    OH, OW = out_hw(H, W)
    P = Bufs()
    xin, g = P.put(x), P.put(dy)
    y = P.out(B * OH * OW * C, x.dtype)
    arg = P.put(torch.full((B * OH * OW * C,), 255, dtype=torch.uint8), fill=170, inout=True)
    dx = P.out(B * H * W * C, x.dtype)
    K.maxpool3s2_fwd(xin.view.view(B, H, W, C), y.view.view(B, OH, OW, C), arg.view.view(B, OH, OW, C))
    P.check(what)
    assert not bool(torch.isnan(dx.view).logical_not().any()), ("the forward wrote dx",) + tuple(what)
    K.maxpool3s2_bwd(g.view.view(B, OH, OW, C), arg.view.view(B, OH, OW, C), dx.view.view(B, H, W, C))
    P.check(what)
    return y.view.view(B, OH, OW, C), arg.view.view(B, OH, OW, C), dx.view.view(B, H, W, C)


def _compare(y, arg, dx, ref, dtype, what):
    assert_same_bits(y.reshape(-1), ref["y"].reshape(-1), ("y",) + what)
    assert_same_bits(arg.reshape(-1), ref["arg"].reshape(-1), ("arg",) + what)
    assert_same_bits(dx.reshape(-1), ref["dx32"].to(dtype).reshape(-1), ("dx",) + what)


@pytest.mark.parametrize("kind", KINDS)
@DT
def test_maxpool(dtype, kind):
    for shape in SHAPES:
        x, dy = pool_inputs(*shape, dtype, kind)
        ref = maxpool_reference(x, dy)
        what = shape + (kind,)
        y, arg, dx = _run(x, dy, what)
        _compare(y, arg, dx, ref, dtype, what)
        # against the float64 sum: exact where one window or none selects the pixel
        got = dx.cpu().double()
        none, once = ref["nsel"] == 0, ref["nsel"] == 1
        assert bool((got[none] == 0).all()) and not bool(torch.signbit(dx.cpu().float()[none]).any()), what
        if dtype == F32:
            assert torch.equal(got[once], ref["dx"][once]), what
            many = ref["nsel"] > 1
            if bool(many.any()):
                mag = float(dy.float().abs().max())
                allow = (ref["nsel"][many] - 1) * U * ref["nsel"][many] * mag
                r = float(((got[many] - ref["dx"][many]).abs() / allow).max())
                key = ("pool dx vs float64, pixels of several windows", dname(dtype))
                RATIOS[key] = max(RATIOS.get(key, 0.0), r)
                assert r <= 1.0, what
        else:
            assert torch.equal(got[once], ref["dx"][once].to(BF16).double()), what


def test_maxpool_past_the_grid_cap():
    """One bf16 ReLU-like input past the cap of 8192 workgroups, forward and backward; inputs and
    reference are made on the device by the same plain slicing code that the CPU tests check."""
    x, dy = pool_inputs(*GRID_CAP_SHAPE, BF16, "relu_bf16", device=DEV)
    ref = maxpool_reference(x, dy, exact64=False)
    y, arg, dx = _run(x, dy, GRID_CAP_SHAPE)
    _compare(y, arg, dx, ref, BF16, GRID_CAP_SHAPE)
    assert int(ref["nsel"].sum()) == dy.numel()


@DT
def test_maxpool_refuses_c12(dtype):
    B, H, W, C = 2, 5, 5, 12
    OH, OW = out_hw(H, W)
    P = Bufs()
    x = P.put(torch.randn(B * H * W * C).to(dtype))
    g = P.put(torch.randn(B * OH * OW * C).to(dtype))
    y, dx = P.out(B * OH * OW * C, dtype), P.out(B * H * W * C, dtype)
    arg = P.put(torch.full((B * OH * OW * C,), 255, dtype=torch.uint8), fill=170, inout=True)
    with pytest.raises(RuntimeError):
        K.maxpool3s2_fwd(x.view.view(B, H, W, C), y.view.view(B, OH, OW, C), arg.view.view(B, OH, OW, C))
    with pytest.raises(RuntimeError):
        K.maxpool3s2_bwd(g.view.view(B, OH, OW, C), arg.view.view(B, OH, OW, C), dx.view.view(B, H, W, C))
    P.check((C,))
    assert bool(torch.isnan(y.view).all()) and bool(torch.isnan(dx.view).all()) and bool((arg.view == 255).all())
