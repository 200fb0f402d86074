"""csrc/kernels/robust.hip through K.robust_rank / robust_gram / robust_krum_select / robust_select_sum
against numpy fp64 (sort, int64 and fp64 Gram matrices), at the smallest shapes with two chunks, a
scalar head and a tail, on both sides of every network size."""
import numpy as np
import pytest
import torch

from psx.ops import kernels as K

pytestmark = pytest.mark.gpu

N, OFF = 2 * 8192 + 13, 3  # the rank kernel's range [OFF, OFF + N): a scalar head, two chunks, a tail
WS = [3, 4, 5, 8, 9, 16, 17, 32]
KINDS = [("trimmed", 1), ("trimmed", 2), ("median", 0)]
CASES = [(k, T, W) for k, T in KINDS for W in WS if k == "median" or W > 2 * T]
DT = {"fp16": torch.float16, "fp32": torch.float32}


def _wires(W, n, dtype, seed=0):
    x = torch.randn(W, n, generator=torch.Generator().manual_seed(seed)).to(dtype)
    x[:, ::10] = x[:2, ::10].repeat(W, 1)[:W]  # ties
    return x


def _rank(x, kind, T, shift=0, order=None):
    """The kernel on the rows of x (CPU [W, n]) over [OFF, OFF + N) of an arena of OFF + N + 5;
    ``shift``: source 0 starts that many elements into its allocation (2 bytes off: the scalar path)."""
    n = OFF + N + 5
    dev = []
    for k in (order if order is not None else range(x.shape[0])):
        buf = torch.zeros(n + 8, dtype=x.dtype, device="cuda")
        s = buf[shift:shift + n] if k == 0 else buf[:n]
        s[OFF:OFF + N] = x[k].cuda()
        dev.append(s)
    agg = torch.full((n,), -7.0, device="cuda")
    K.robust_rank(dev, agg, kind, trim=T, n=n, off=OFF, cnt=N)
    out = agg.cpu()
    assert bool((out[:OFF] == -7.0).all()) and bool((out[OFF + N:] == -7.0).all())  # nothing outside the range
    return out[OFF:OFF + N]


def _check(got, x, kind, T):
    W = x.shape[0]
    xs = x.double().numpy()
    s = np.sort(np.where(np.isnan(xs), np.inf, xs), axis=0)
    g = got.double().numpy()
    if kind == "median":
        # fp16 wires: a + b of two halves is exact in fp32, so is the halving; fp32 wires: one fp32 add
        want = np.float32(0.5) * (s[W // 2 - 1].astype(np.float32) + s[W // 2].astype(np.float32)) if W % 2 == 0 \
            else s[(W - 1) // 2]
        assert (g == want).all()
    else:
        kept = s[T:W - T]
        # m = W - 2T kept values, S = sum |kept|, u = 2^-24. The chain from 0 has m - 1 rounding adds (0 + x is exact),
        # each off by <= u * S: the sum is within (m - 1) u S, the mean within (m - 1) u S / m. The multiply by
        # fl(1 / m) adds two relative u of |mean| <= S / m. Together (m + 1) u S / m <= m u S for m >= 2; m = 1 is exact.
        bound = (W - 2 * T) * 2.0 ** -24 * np.abs(kept).sum(axis=0)
        fin = np.isfinite(kept).all(axis=0)
        assert (np.abs(g[fin] - kept.mean(axis=0)[fin]) <= bound[fin]).all()
        assert (g[~fin] == np.inf).all()


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
@pytest.mark.parametrize("kind,T,W", CASES)
def test_rank_kernel_against_fp64_sort_and_is_permutation_invariant(kind, T, W, wire):
    x = _wires(W, N, DT[wire], seed=W)
    got = _rank(x, kind, T)
    _check(got, x, kind, T)
    assert bool((_rank(x, kind, T, order=range(W - 1, -1, -1)) == got).all())  # by value: -0 == +0


@pytest.mark.parametrize("kind,T,W", [("trimmed", 1, 5), ("median", 0, 17)])
def test_rank_kernel_unaligned_source_takes_the_scalar_path(kind, T, W):
    x = _wires(W, N, torch.float16, seed=40 + W)
    got = _rank(x, kind, T, shift=1)
    _check(got, x, kind, T)
    assert bool((got == _rank(x, kind, T)).all())


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("W", [5, 9])
def test_rank_kernel_one_contaminated_source(W, bad, wire):
    x = _wires(W, N, DT[wire], seed=60 + W)
    x[2] = bad
    got = _rank(x, "trimmed", 1)
    _check(got, x, "trimmed", 1)  # the reference sorts with NaN replaced by +inf
    assert bool(torch.isfinite(got).all())


def _int_wires(W, n, dtype, seed):
    return torch.randint(-8, 9, (W, n), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _gram(x):
    st = K.KrumState(x.shape[1], "cuda")
    K.robust_gram(list(x.cuda()), st)
    return st, st.partials.double().sum(0).cpu().numpy()


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
@pytest.mark.parametrize("W", [5, 7, 16, 17, 32])
def test_gram_of_small_integers_is_exact(W, wire):
    x = _int_wires(W, 20_000 + 5, DT[wire], seed=W)  # |x| <= 8: every product and partial sum is exact in fp32
    xi = x.long().numpy()
    G = _gram(x)[1]
    iu = np.triu_indices(W)
    assert (G[:W, :W][iu] == (xi @ xi.T)[iu]).all()


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
def test_gram_of_random_values_within_the_chain_bound(wire):
    x = torch.randn(17, 20_000 + 5, generator=torch.Generator().manual_seed(3)).to(DT[wire])
    xd = x.double().numpy()
    G = _gram(x)[1]
    # a partial sums at most L = ROBUST_GRAM_SLICE products in fp32, in any order: <= L * 2^-24 * sum |a_i b_i|; the
    # partials are then added in double
    bound = K.ROBUST_GRAM_SLICE * 2.0 ** -24 * (np.abs(xd) @ np.abs(xd).T)
    iu = np.triu_indices(17)
    assert (np.abs(G[:17, :17] - xd @ xd.T)[iu] <= bound[iu]).all()


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
def test_krum_selects_the_honest_five(wire):
    W, F, n = 7, 2, 20_000 + 5
    base = _int_wires(1, n, torch.float32, seed=5)[0].clamp(-2, 2)
    x = torch.stack([base + _int_wires(1, n, torch.float32, seed=10 + k)[0].clamp(-1, 1) for k in range(5)]
                    + [-4 * base, -4 * base]).to(DT[wire])
    xi = x.long().numpy()
    Gi = xi @ xi.T
    d2 = np.diag(Gi)[:, None] + np.diag(Gi)[None, :] - 2 * Gi
    score = np.array([np.sort(np.delete(d2[i], i))[: W - F - 2].sum() for i in range(W)])
    assert score[5:].min() - score[:5].max() > 0  # the inputs themselves: the two outliers score worst
    st, _ = _gram(x)
    for _ in range(2):
        sel = K.robust_krum_select(st, W, F)
    assert sel.cpu().tolist() == [1.0] * 5 + [0.0] * (32 - 5)
    assert st.selected.cpu().tolist() == [2] * 5 + [0] * (32 - 5)
    agg = torch.empty(n, device="cuda")
    K.robust_select_sum(list(x.cuda()), st, agg, W - F)
    xd = x[:5].double().numpy()
    assert (np.abs(agg.double().cpu().numpy() - xd.mean(0)) <= 5 * 2.0 ** -24 * np.abs(xd).sum(0)).all()

