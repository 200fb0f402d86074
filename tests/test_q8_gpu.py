"""The q8 gradient codec's HIP kernels (csrc/kernels/q8.hip) against the torch CPU path of
parallel/q8.py (bit for bit) and against the dense update kernels, plus a loopback run."""
import pytest
import torch

from psx.ops import kernels as K
from psx.ops._lib import HipError
from psx.parallel import q8 as Q

from .test_q8_cpu import check_step, make_grads

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [255, 256, 257, 4097, 1_000_003]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of two fp32 tensors (NaNs included)."""
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n", SIZES)
def test_encode_matches_cpu(n, dtype):
    assert K.q8_payload_bytes(n) == Q.payload_bytes(n)
    cpu, gpu = Q.Q8Codec(n), Q.Q8Codec(n, DEV)
    for g in make_grads(n, dtype):
        acc = cpu.resid + g.float()
        pc = cpu.encode(g)
        pg = gpu.encode(g.to(DEV))
        assert torch.equal(pg.cpu(), pc)
        assert _same(gpu.resid, cpu.resid)
        check_step(acc, pg.cpu(), gpu.resid.cpu(), n)


def test_zero_and_nonfinite_blocks():
    n = 4097
    cpu, gpu = Q.Q8Codec(n), Q.Q8Codec(n, DEV)
    for g in make_grads(n, torch.float32, special=True):
        acc = cpu.resid + g.float()
        pc, pg = cpu.encode(g), gpu.encode(g.to(DEV))
        # NaN scales / residuals may differ in payload bits only; compare through the views
        for a, b in zip(Q.views(pg.cpu(), n), Q.views(pc, n)):
            assert torch.equal(a.isnan(), b.isnan()) if a.is_floating_point() else torch.equal(a, b)
            if a.is_floating_point():
                assert torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
        assert torch.equal(gpu.resid.cpu().isnan(), cpu.resid.isnan())
        assert torch.equal(gpu.resid.cpu().nan_to_num(0.0), cpu.resid.nan_to_num(0.0))
        check_step(acc, pg.cpu(), gpu.resid.cpu(), n)
        dec, dec_ref = Q.decode(pg, n).cpu(), Q.decode(pc, n)
        assert torch.equal(dec.isnan(), dec_ref.isnan()) and torch.equal(dec.nan_to_num(0.0), dec_ref.nan_to_num(0.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("offset", [0, 1])
def test_encode_guards(offset, dtype):
    """n = 257 (a full block and a one-element tail block) on slices that end exactly at their
    allocation's end, at offset 1 on the element-wise path; guard bands after resid and after the
    payload, and the element before the slices, stay untouched."""
    n, band = 257, 64
    g_cpu = make_grads(n, dtype, steps=1, seed=9)[0]
    r_cpu = make_grads(n, torch.float32, steps=1, seed=11)[0]
    ref = Q.Q8Codec(n)
    ref.resid.copy_(r_cpu)
    ref.encode(g_cpu)
    # slices ending at the end of their allocations
    g_end = torch.zeros(offset + n, dtype=dtype, device=DEV)
    r_end = torch.zeros(offset + n, device=DEV)
    g_end[offset:] = g_cpu.to(DEV)
    r_end[offset:] = r_cpu.to(DEV)
    p_end = Q.empty_payload(n, DEV)
    K.q8_encode(g_end[offset:], r_end[offset:], p_end, n)
    assert torch.equal(p_end.cpu(), ref.payload) and _same(r_end[offset:], ref.resid)
    # guard bands
    pb = Q.payload_bytes(n)
    r_big = torch.full((offset + n + band,), 77.0, device=DEV)
    r_big[offset:offset + n] = r_cpu.to(DEV)
    p_big = torch.full((pb + band,), 0xAB, dtype=torch.uint8, device=DEV)
    p_big[:pb] = 0
    K.q8_encode(g_end[offset:], r_big[offset:offset + n], p_big[:pb], n)
    assert torch.equal(p_big[:pb].cpu(), ref.payload) and _same(r_big[offset:offset + n], ref.resid)
    assert bool((r_big[offset + n:] == 77.0).all()) and bool((r_big[:offset] == 77.0).all())
    assert bool((p_big[pb:] == 0xAB).all())
    assert torch.equal(g_end[offset:].cpu(), g_cpu)


def _payloads(n: int, W: int):
    """W encoded payloads of distinct seeded gradients on the device, built once per (n, W)."""
    key = (n, W)
    if key not in _payloads.cache:
        enc = Q.Q8Codec(n, DEV)
        out = []
        for k in range(W):
            g = make_grads(n, torch.float32, steps=1, seed=100 + k)[0].to(DEV)
            out.append(enc.encode(g).clone())
            enc.resid.zero_()
        _payloads.cache[key] = out
    return _payloads.cache[key]


_payloads.cache = {}


def test_payload_over_the_state_is_refused():
    """A payload that shares a byte with what the call writes is refused with hipErrorInvalidValue
    before anything is launched: q8_apply_multi with a payload that is a view of p's own storage,
    q8_decode with dst over the payload (n = 257). p and dst keep their bits."""
    n = 257
    pb = Q.payload_bytes(n)
    payload = Q.Q8Codec(n).encode(make_grads(n, torch.float32, steps=1, seed=3)[0])
    p = torch.randn(n, device=DEV)
    inside = p.view(torch.uint8)[:pb]
    inside.copy_(payload.to(DEV))
    before = p.clone()
    with pytest.raises(HipError, match="q8_apply_multi failed with code 1$"):
        K.q8_apply_multi(p, [inside], 0.1, n=n)
    torch.cuda.synchronize()
    assert _same(p, before)
    store = torch.zeros(4 * n, dtype=torch.uint8, device=DEV)
    store[:pb] = payload.to(DEV)
    dst, before = store.view(torch.float32), store.clone()
    with pytest.raises(HipError, match="q8_decode failed with code 1$"):
        K.q8_decode(store[:pb], dst, n)
    torch.cuda.synchronize()
    assert torch.equal(store, before)


@pytest.mark.parametrize("n", [257, 4097, 1_000_003])
def test_decode_matches_cpu(n):
    p = _payloads(n, 1)[0]
    pc = p.cpu()
    assert _same(Q.decode(p, n), Q.decode(pc, n))
    base = make_grads(n, torch.float32, steps=1, seed=21)[0]
    for off in (0, 1):  # 16-byte aligned and element-wise destination
        big = torch.zeros(off + n, device=DEV)
        big[off:] = base.to(DEV)
        K.q8_decode(p, big[off:], n, scale=0.37, add=True)
        assert _same(big[off:], Q.decode(pc, n, out=base.clone(), scale=0.37, add=True))
        K.q8_decode(p, big[off:], n, scale=-2.5, add=False)
        assert _same(big[off:], Q.decode(pc, n, scale=-2.5))


VARIANTS = {"plain": dict(momentum=0.0, wd=0.0, first=False), "mom_first": dict(momentum=0.9, wd=0.0, first=True),
            "mom": dict(momentum=0.9, wd=0.0, first=False), "wd": dict(momentum=0.0, wd=5e-4, first=False)}


@pytest.mark.parametrize("with_img", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("W", [1, 3, 32])
@pytest.mark.parametrize("n", [257, 4097, 1_000_003])
def test_apply_multi(n, W, variant, with_img):
    """(a) bit-equal to sgd_apply on the dense fp32 sum built by chained q8_decode(add=True) in
    source order (what a loopback round computes); (b) close to an fp64 evaluation: rtol 1e-6 of
    the result (its own final rounding) plus the propagated rounding of d — 2 W + 8 roundings of
    at most 2^-24 each (W products, W adds, the gscale / weight-decay / momentum multiplies, and
    lr, gscale, wd, momentum themselves as fp32) on lr * (gscale sum|deq| + wd |p| +
    momentum |buf|); (c) img == params.bfloat16()."""
    v = VARIANTS[variant]
    lr, gscale = 0.1, 1.0 / W
    srcs = _payloads(n, W)
    p0 = make_grads(n, torch.float32, steps=1, seed=31)[0].to(DEV) * 1e3  # ~N(0, 1)
    b0 = make_grads(n, torch.float32, steps=1, seed=32)[0].to(DEV)
    mom = v["momentum"] != 0.0
    p1, p2 = p0.clone(), p0.clone()
    buf1, buf2 = (b0.clone(), b0.clone()) if mom else (None, None)
    img1 = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if with_img else None
    img2 = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if with_img else None
    K.q8_apply_multi(p1, srcs, lr, gscale=gscale, buf=buf1, n=n, img=img1, **v)
    dense = torch.zeros(n, device=DEV)
    for s in srcs:
        K.q8_decode(s, dense, n, add=True)
    K.sgd_apply(p2, dense, lr, gscale=gscale, buf=buf2, n=n, img=img2, **v)
    assert _same(p1, p2)
    if mom:
        assert _same(buf1, buf2)
    if with_img:
        assert torch.equal(img1.view(torch.int16), p1.bfloat16().view(torch.int16))
        assert torch.equal(img1.view(torch.int16), img2.view(torch.int16))
    # fp64 evaluation
    deq = torch.stack([Q.decode(s, n).double() for s in srcs])
    d = gscale * deq.sum(0) + v["wd"] * p0.double()
    mag = gscale * deq.abs().sum(0) + v["wd"] * p0.double().abs()
    if mom and not v["first"]:
        d = v["momentum"] * b0.double() + d
        mag = v["momentum"] * b0.double().abs() + mag
    ref = p0.double() - lr * d
    bound = 1e-6 * ref.abs() + (2 * W + 8) * 2.0 ** -24 * lr * mag
    assert bool(((p1.double() - ref).abs() <= bound).all())


def test_apply_multi_unaligned_matches_aligned():
    """The element-wise form (a parameter slice at an odd element offset) gives the same bits."""
    n, W = 4097, 3
    srcs = _payloads(n, W)
    p0 = make_grads(n, torch.float32, steps=1, seed=31)[0].to(DEV) * 1e3
    a = p0.clone()
    big = torch.zeros(1 + n, device=DEV)
    big[1:] = p0
    K.q8_apply_multi(a, srcs, 0.1, gscale=1 / 3, wd=5e-4, n=n)
    K.q8_apply_multi(big[1:], srcs, 0.1, gscale=1 / 3, wd=5e-4, n=n)
    assert _same(a, big[1:])


def test_subrange_matches_whole():
    n, cut = 4097, 2048
    g = make_grads(n, torch.float16, steps=1, seed=41)[0].to(DEV)
    whole, parts = Q.Q8Codec(n, DEV), Q.Q8Codec(n, DEV)
    whole.encode(g)
    Q.encode_into(g, parts.resid, parts.payload, n, 0, cut)
    Q.encode_into(g, parts.resid, parts.payload, n, cut, n - cut)
    assert torch.equal(whole.payload, parts.payload) and _same(whole.resid, parts.resid)
    srcs = _payloads(n, 3)
    p0 = make_grads(n, torch.float32, steps=1, seed=31)[0].to(DEV) * 1e3
    a, b = p0.clone(), p0.clone()
    ba, bb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ia, ib = (torch.zeros(n, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    kw = dict(gscale=1 / 3, momentum=0.9, wd=5e-4, first=True, n=n)
    K.q8_apply_multi(a, srcs, 0.1, buf=ba, img=ia, **kw)
    K.q8_apply_multi(b, srcs, 0.1, buf=bb, img=ib, off=0, cnt=cut, **kw)
    assert _same(b[cut:], p0[cut:]) and not bool(ib[cut:].any())  # the rest is untouched
    K.q8_apply_multi(b, srcs, 0.1, buf=bb, img=ib, off=cut, cnt=n - cut, **kw)
    assert _same(a, b) and _same(ba, bb) and torch.equal(ia.view(torch.int16), ib.view(torch.int16))
    out = torch.full((n,), 3.0, device=DEV)
    K.q8_decode(srcs[0], out, n, add=True, off=cut, cnt=n - cut)
    assert bool((out[:cut] == 3.0).all()) and _same(out[cut:], (Q.decode(srcs[0], n) + 3.0)[cut:])
    with pytest.raises(AssertionError):
        K.q8_decode(srcs[0], out, n, off=100, cnt=256)


def test_loopback_run_is_deterministic():
    from psx.parallel.runner import run_local
    from psx.utils.config import PSConfig

    shas = []
    for _ in range(2):
        cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.1,
                       max_steps=4, mode="sync", workers=2, codec="q8", deterministic=True).validate()
        srv = run_local(cfg, log=lambda *a, **k: None)["server"]
        assert srv["global_steps_completed"] == 4 and srv["gradients_processed"] == 8
        assert srv["final_param_checksum"] == srv["final_param_checksum"]  # not NaN
        shas.append(srv["final_param_sha256"])
    assert shas[0] == shas[1]
