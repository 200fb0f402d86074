"""The delta fetch wire's encode kernel (csrc/kernels/q8.hip fetchq8_encode) against the torch CPU
path of parallel/fetchq8.py, bit for bit, on the payload and on the new shadow; its bounds; and the
worker-side add (q8_decode) against the shadow over several rounds."""
import pytest
import torch

from psx.ops import kernels as K
from psx.parallel import fetchq8 as F
from psx.parallel import q8 as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [255, 256, 257, 4097, 1_000_003]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of two fp32 tensors (NaNs included)."""
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _rounds(n: int, rounds: int, seed: int = 0):
    """(initial state, [arena after each round]) on the CPU: weights of size 0.05 that move by
    1e-3 a round, one element in a hundred ten times as far."""
    if (n, rounds, seed) not in _rounds.cache:
        g = torch.Generator().manual_seed(4321 + n + seed)
        base = torch.randn(n, generator=g) * 0.05
        arena, out = base.clone(), []
        for _ in range(rounds):
            step = torch.randn(n, generator=g) * 1e-3
            arena = arena - torch.where(torch.rand(n, generator=g) < 0.01, step * 10.0, step)
            out.append(arena)
        _rounds.cache[(n, rounds, seed)] = (base, out)
    return _rounds.cache[(n, rounds, seed)]


_rounds.cache = {}


def _on_device(t: torch.Tensor, offset: int) -> torch.Tensor:
    """A device copy of t that starts ``offset`` elements into its allocation (offset 1: not
    16-byte aligned, the element-wise form) and ends at the allocation's end."""
    buf = torch.zeros(offset + t.numel(), dtype=t.dtype, device=DEV)
    buf[offset:] = t.to(DEV)
    return buf[offset:]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_encode_matches_cpu(n, offset):
    base, arenas = _rounds(n, 2)
    sh_c, pl_c = base.clone(), Q.empty_payload(n, "cpu")
    sh_g, pl_g = _on_device(base, offset), Q.empty_payload(n, DEV)
    for a in arenas:
        F.encode_into(a, sh_c, pl_c, n)
        F.encode_into(_on_device(a, offset), sh_g, pl_g, n)
        assert torch.equal(pl_g.cpu(), pl_c)
        assert _same(sh_g, sh_c)


@pytest.mark.parametrize("offset", [0, 1])
def test_encode_guards(offset):
    """n = 257 (a full block and a one-element tail block) on slices that end exactly at their
    allocation's end; guard bands after the shadow and after the payload, and the element before
    the slices, stay untouched, and the arena is only read."""
    n, band = 257, 64
    base, (a_cpu,) = _rounds(n, 1, seed=9)
    ref_s, ref_p = base.clone(), Q.empty_payload(n, "cpu")
    F.encode_into(a_cpu, ref_s, ref_p, n)
    a_end = _on_device(a_cpu, offset)
    pb = Q.payload_bytes(n)
    s_big = torch.full((offset + n + band,), 77.0, device=DEV)
    s_big[offset:offset + n] = base.to(DEV)
    p_big = torch.full((pb + band,), 0xAB, dtype=torch.uint8, device=DEV)
    p_big[:pb] = 0
    K.fetchq8_encode(a_end, s_big[offset:offset + n], p_big[:pb], n)
    assert torch.equal(p_big[:pb].cpu(), ref_p) and _same(s_big[offset:offset + n], ref_s)
    assert bool((s_big[offset + n:] == 77.0).all()) and bool((s_big[:offset] == 77.0).all())
    assert bool((p_big[pb:] == 0xAB).all())
    assert _same(a_end, a_cpu)
    # and with the shadow itself ending at its allocation's end
    s_end = _on_device(base, offset)
    p_end = Q.empty_payload(n, DEV)
    K.fetchq8_encode(a_end, s_end, p_end, n)
    assert torch.equal(p_end.cpu(), ref_p) and _same(s_end, ref_s)


def test_zero_and_nonfinite_blocks():
    n = 4097
    base, (a_cpu,) = _rounds(n, 1, seed=5)
    a_cpu = a_cpu.clone()
    a_cpu[:256] = base[:256]          # block 0: nothing changed
    a_cpu[300] = float("nan")         # block 1
    a_cpu[700] = float("inf")         # block 2
    a_cpu[4096] = float("-inf")       # the tail block
    sh_c, pl_c = base.clone(), Q.empty_payload(n, "cpu")
    sh_g, pl_g = base.to(DEV), Q.empty_payload(n, DEV)
    for _ in range(2):  # the second round starts from NaN blocks in the shadow
        F.encode_into(a_cpu, sh_c, pl_c, n)
        F.encode_into(a_cpu.to(DEV), sh_g, pl_g, n)
        # NaN scales may differ in their payload bits only; compare through the views
        for a, b in zip(Q.views(pl_g.cpu(), n), Q.views(pl_c, n)):
            if a.is_floating_point():
                assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))
            else:
                assert torch.equal(a, b)
        got = sh_g.cpu()
        assert torch.equal(got.isnan(), sh_c.isnan()) and _same(got.nan_to_num(0.0), sh_c.nan_to_num(0.0))
        _, scales, q = Q.views(pl_g.cpu(), n)
        assert float(scales[0]) == 0.0 and int(q[:256].abs().sum()) == 0 and _same(got[:256], base[:256])
        assert bool(scales[[1, 2, 16]].isnan().all()) and bool(scales[3:16].isfinite().all())
        assert bool(got[256:768].isnan().all()) and bool(got[4096:].isnan().all())
        assert bool(got[768:4096].isfinite().all())


def test_subrange_equals_whole():
    n = 4097
    base, (a_cpu,) = _rounds(n, 1, seed=2)
    a = a_cpu.to(DEV)
    sh_w, pl_w = base.to(DEV), Q.empty_payload(n, DEV)
    K.fetchq8_encode(a, sh_w, pl_w, n)
    for off, cnt in ((512, 1024), (3840, 257), (0, 256)):
        sh_p, pl_p = base.to(DEV), Q.empty_payload(n, DEV)
        K.fetchq8_encode(a, sh_p, pl_p, n, off, cnt)
        assert _same(sh_p[off:off + cnt], sh_w[off:off + cnt])
        assert _same(sh_p[:off], base[:off]) and _same(sh_p[off + cnt:], base[off + cnt:])
        (_, sw, qw), (_, sp, qp) = Q.views(pl_w, n), Q.views(pl_p, n)
        b0, b1 = off // 256, -(-(off + cnt) // 256)
        assert torch.equal(qp[off:off + cnt], qw[off:off + cnt]) and _same(sp[b0:b1], sw[b0:b1])
        assert int(qp[:off].abs().sum()) == 0 and int(qp[off + cnt:].abs().sum()) == 0
    with pytest.raises(AssertionError):
        K.fetchq8_encode(a, sh_w, pl_w, n, 100, 256)


@pytest.mark.parametrize("n", [4097, 1_000_003])
def test_five_rounds_worker_equals_shadow(n):
    """A worker buffer that only ever receives the decode-add of the payloads equals the shadow
    bit for bit after every round, and both equal the CPU path's shadow."""
    base, arenas = _rounds(n, 5, seed=1)
    sh_c, pl_c = base.clone(), Q.empty_payload(n, "cpu")
    sh_g, pl_g, worker = base.to(DEV), Q.empty_payload(n, DEV), base.to(DEV)
    for a in arenas:
        F.encode_into(a, sh_c, pl_c, n)
        F.encode_into(a.to(DEV), sh_g, pl_g, n)
        F.apply(pl_g, worker, n)
        assert _same(worker, sh_g) and _same(sh_g, sh_c)
