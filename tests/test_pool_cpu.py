"""The reference of the 3x3 / stride-2 / pad-1 max-pool (csrc/kernels/pool.hip), forward and
backward, and the CPU tests that show it is right: on inputs without ties it equals torch's CPU
max_pool2d forward, indices and backward; on tied inputs the first maximum in window order wins
and the padding, which is skipped and not read as zero, never does. ``maxpool_reference`` and
``pool_inputs`` are shared with tests/test_pool_gpu.py.

The backward of the kernel is a gather: input pixel (2m + dh, 2n + dw) adds, in fp32 and in the
order (doh, dow) = (0, 0), (0, 1), (1, 0), (1, 1), the gradients of the outputs (m + doh, n + dow)
whose recorded tap is (dh + 1 - 2 doh, dw + 1 - 2 dow). ``dx32`` repeats exactly those adds (adding
+0 where the tap differs changes no bits: the accumulator starts at +0 and is never -0), so the
kernel's fp32 dx must equal it bit for bit and its bf16 dx must be its bf16 rounding; ``dx`` is the
same sum in float64 and ``nsel`` the number of windows that selected the pixel."""
import pytest
import torch
import torch.nn.functional as F

from .test_bn_cpu import BF16, F32
from .test_sgd_cpu import U

KINDS = ("randn", "relu_bf16", "constant", "negative")
SHAPES = ((1, 1, 1, 8), (2, 2, 1, 8), (3, 7, 9, 16), (2, 16, 16, 64))  # (B, H, W, C)
GRID_CAP_SHAPE = (3, 224, 224, 512)  # B OH OW C / 8 > 8192 x 256: the second grid-stride trip
GRID_CAP = 8192 * 256


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_inputs(B, H, W, C, dtype, kind, device="cpu"):
    """(x, dy) of ``dtype``. randn: no ties; relu_bf16: a ReLU output on the bf16 grid, about half
    zeros; constant: every window fully tied; negative: every value below zero."""
    gen = torch.Generator(device=device).manual_seed(211 + B + 3 * H + 5 * W + 7 * C + 11 * KINDS.index(kind))
    r = torch.randn(B, H, W, C, generator=gen, device=device)
    OH, OW = out_hw(H, W)
    dy = torch.randn(B, OH, OW, C, generator=gen, device=device).to(dtype)
    if kind == "relu_bf16":
        r = torch.relu(r).to(BF16).float()
    elif kind == "constant":
        r = torch.full_like(r, 1.5)
    elif kind == "negative":
        r = -r.abs() - 0.125
    return r.to(dtype), dy


def maxpool_reference(x, dy=None, exact64=True):
    """x [B, H, W, C] -> dict: y (x's dtype: the maximum itself), arg (uint8, the first strict
    maximum among the nine taps r * 3 + s in window order, taps in the padding skipped) and, given
    dy: dx32 (the kernel's fp32 adds in its order), nsel, and with ``exact64`` dx (float64). Plain
    torch slicing, on x's device."""
    B, H, W, C = x.shape
    OH, OW = out_hw(H, W)
    xf = F.pad(x.float(), (0, 0, 1, 1, 1, 1))  # values are never compared where valid is false
    valid = F.pad(torch.ones(1, H, W, 1, dtype=torch.bool, device=x.device), (0, 0, 1, 1, 1, 1))
    best = torch.full((B, OH, OW, C), float("-inf"), device=x.device)
    arg = torch.zeros((B, OH, OW, C), dtype=torch.uint8, device=x.device)
    for r in range(3):
        for s in range(3):  # padded row 2 oh + r is input row 2 oh - 1 + r
            v = xf[:, r:r + 2 * OH:2, s:s + 2 * OW:2][:, :OH, :OW]
            ok = valid[:, r:r + 2 * OH:2, s:s + 2 * OW:2][:, :OH, :OW]
            upd = ok & (v > best)
            best = torch.where(upd, v, best)
            arg = torch.where(upd, torch.full_like(arg, r * 3 + s), arg)
    out = dict(y=best.to(x.dtype), arg=arg)
    if dy is None:
        return out
    dx32 = torch.zeros(B, H, W, C, device=x.device)
    nsel = torch.zeros(B, H, W, C, dtype=torch.int32, device=x.device)
    dx64 = torch.zeros(B, H, W, C, dtype=torch.float64, device=x.device) if exact64 else None
    g32 = dy.float()
    for doh in range(2):
        for dow in range(2):
            for dh in range(2):
                for dw in range(2):
                    r, s = dh + 1 - 2 * doh, dw + 1 - 2 * dow
                    if r < 0 or s < 0:
                        continue
                    # pixels (2 m + dh, 2 n + dw) with output (m + doh, n + dow) in range
                    nm = min((H - dh + 1) // 2, OH - doh)
                    nn = min((W - dw + 1) // 2, OW - dow)
                    if nm <= 0 or nn <= 0:
                        continue
                    sel = arg[:, doh:doh + nm, dow:dow + nn] == r * 3 + s
                    gg = g32[:, doh:doh + nm, dow:dow + nn]
                    ih, iw = slice(dh, dh + 2 * nm, 2), slice(dw, dw + 2 * nn, 2)
                    dx32[:, ih, iw] = dx32[:, ih, iw] + torch.where(sel, gg, torch.zeros_like(gg))
                    nsel[:, ih, iw] += sel.int()
                    if exact64:
                        dx64[:, ih, iw] += torch.where(sel, gg.double(), torch.zeros_like(gg, dtype=torch.float64))
    out.update(dx32=dx32, nsel=nsel)
    if exact64:
        out["dx"] = dx64
    return out


def _torch_pool(x, dy):
    xt = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    y, idx = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    y.backward(dy.double().permute(0, 3, 1, 2))
    back = lambda t: t.permute(0, 2, 3, 1)
    return back(y.detach()), back(idx), back(xt.grad)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_reference_equals_torch_without_ties(dtype):
    for shape in SHAPES + ((2, 5, 4, 8), (1, 2, 2, 8)):
        B, H, W, C = shape
        x, dy = pool_inputs(*shape, F32, "randn")
        if dtype == BF16:  # rounding randn to bf16 would tie values: distinct bit patterns, both signs
            i = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(1)).view(x.shape)
            word = 0x1000 + (i >> 1) + ((i & 1) << 15)
            x = torch.where(word >= 32768, word - 65536, word).to(torch.int16).view(BF16)
            assert x.unique().numel() == x.numel() and bool(torch.isfinite(x.float()).all())
            dy = dy.to(BF16)
        ref = maxpool_reference(x, dy)
        y, idx, dx = _torch_pool(x, dy)
        OH, OW = out_hw(H, W)
        assert torch.equal(ref["y"].double(), y), shape
        a = ref["arg"].long()
        oh = torch.arange(OH).view(1, OH, 1, 1)
        ow = torch.arange(OW).view(1, 1, OW, 1)
        flat = (2 * oh - 1 + a // 3) * W + 2 * ow - 1 + a % 3
        assert torch.equal(flat, idx), shape
        assert torch.equal(ref["dx"], dx), shape  # float64 sums of at most four fp32 values: exact
        assert float((ref["dx32"].double() - dx).abs().max()) <= 3 * U * float(dy.float().abs().max()) * 4


def test_first_maximum_wins_and_padding_never_does():
    for shape in SHAPES:
        B, H, W, C = shape
        OH, OW = out_hw(H, W)
        x, dy = pool_inputs(*shape, F32, "constant")
        ref = maxpool_reference(x, dy)
        # the first tap inside the image: row tap 1 for oh = 0 (tap 0 is padding), else 0
        r0 = (torch.arange(OH) == 0).long().view(1, OH, 1, 1)
        s0 = (torch.arange(OW) == 0).long().view(1, 1, OW, 1)
        assert torch.equal(ref["arg"].long(), (r0 * 3 + s0).expand(B, OH, OW, C)), shape
        assert bool((ref["y"] == 1.5).all())
        x, dy = pool_inputs(*shape, F32, "negative")
        ref = maxpool_reference(x, dy)
        assert bool((ref["y"] < 0).all()), shape
        y, _, dx = _torch_pool(x, dy)
        assert torch.equal(ref["y"].double(), y) and torch.equal(ref["dx"], dx), shape
        # a ReLU output on the bf16 grid: ties are the rule; every gradient lands exactly once
        x, dy = pool_inputs(*shape, BF16, "relu_bf16")
        ref = maxpool_reference(x, dy)
        assert int(ref["nsel"].sum()) == dy.numel(), shape
        assert abs(float(ref["dx"].sum()) - float(dy.double().sum())) <= 1e-9 * dy.numel()
        if x.numel() >= 1000:
            assert 0.3 < float((x == 0).float().mean()) < 0.7
        # the tap recorded holds the maximum, and no earlier tap inside the image does
        xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1), value=float("-inf"))
        for t in range(9):
            r, s = divmod(t, 3)
            v = xp[:, r:r + 2 * OH:2, s:s + 2 * OW:2][:, :OH, :OW]
            assert bool((v <= ref["y"].float()).all())
            assert bool((v[ref["arg"] == t] == ref["y"].float()[ref["arg"] == t]).all())
            assert bool((v[ref["arg"] > t] < ref["y"].float()[ref["arg"] > t]).all()), (shape, t)


def test_dx32_is_the_sum_within_its_roundings():
    for shape in SHAPES:
        for kind in KINDS:
            x, dy = pool_inputs(*shape, F32, kind)
            ref = maxpool_reference(x, dy)
            once = ref["nsel"] <= 1
            assert torch.equal(ref["dx32"][once].double(), ref["dx"][once]), (shape, kind)
            assert bool((ref["dx"][ref["nsel"] == 0] == 0).all())
            mag = float(dy.float().abs().max())
            err = (ref["dx32"].double() - ref["dx"]).abs()
            assert bool((err <= (ref["nsel"] - 1).clamp_min(0) * U * ref["nsel"] * mag).all()), (shape, kind)


def test_grid_cap_shape_and_host_refusals():
    B, H, W, C = GRID_CAP_SHAPE
    OH, OW = out_hw(H, W)
    assert B * OH * OW * C // 8 > GRID_CAP and B * ((H + 1) // 2) * ((W + 1) // 2) * C // 8 > GRID_CAP
    for shape in SHAPES:
        assert shape[0] * out_hw(shape[1], shape[2])[0] * out_hw(shape[1], shape[2])[1] * shape[3] // 8 <= GRID_CAP
    # refusals return before any launch: C % 8, and an index that would pass 2^31
    from psx.ops._lib import kernels
    for f32_ in (0, 1):
        for fn in (kernels().psx_maxpool3s2_fwd, kernels().psx_maxpool3s2_bwd):
            assert fn(None, None, None, 2, 8, 8, 12, f32_, None) == -2
            assert fn(None, None, None, 4096, 64, 64, 4096, f32_, None) == -2  # 2^31 vectors of 8 channels
            assert fn(None, None, None, 4096 - 4, 64, 64, 4096, f32_, None) == -2  # 2^31 - 2^21: the stride's room
