"""csrc/kernels/robust_iter.hip through K.robust_iter_step / robust_iter_weights and Robust.combine
against numpy int64 / fp64: two chunks, one 8-group and a scalar tail in the last, both sides of every
register-file size, both wire types."""
import numpy as np
import pytest
import torch

from psx.ops import kernels as K
from psx.parallel import robust as RB
from psx.utils.config import PSConfig

from .test_robust_iter_cpu import U, contaminated, ref64
from .test_robust_server_gpu import _drive, _server

pytestmark = pytest.mark.gpu

N = 2 * 8192 + 13
DT = {"fp16": torch.float16, "fp32": torch.float32}


def _pass(kind, centre, W, wire, shift=0, nan=None, seed=0):
    """One pass over integer wires in [-4, 4] with a_k from {0, 1/8, 1/4}, b from {1, 1/2} and an integer
    centre: every product, sum, square and lane chain is exact in fp32. Returns what the kernel left
    (centre, per-source sums of the partials, agg) and the same from fp64 numpy."""
    gen = torch.Generator().manual_seed(100 * W + seed)
    x = torch.randint(-4, 5, (W, N), generator=gen).to(DT[wire])
    a = torch.randint(0, 3, (W,), generator=gen).double().numpy() / 8.0
    b = 1.0 / float(torch.randint(1, 3, (1,), generator=gen))
    v0 = torch.randint(-4, 5, (N,), generator=gen).float()
    if nan is not None:
        x[nan], a[nan] = float("nan"), 0.0
    st = K.RobustIterState(N, "cuda", centre=centre)
    if centre:
        st.centre.copy_(v0)
    dev = []
    for k in range(W):  # source 0 `shift` elements into its allocation: 2 bytes off takes the scalar path
        buf = torch.zeros(N + 8, dtype=x.dtype, device="cuda")
        dev.append(buf[shift:shift + N] if k == 0 else buf[:N])
        dev[-1].copy_(x[k])
    agg = torch.full((N + 5,), -7.0, device="cuda")
    K.robust_iter_step(dev, st, kind, agg=agg, c=0.5, weights=(a, b))
    xd, s = x.double().numpy(), (v0.double().numpy() if centre else np.zeros(N))
    if kind != "init":
        s = (b * s if centre else 0.0) + sum(a[k] * xd[k] for k in range(W) if a[k] != 0.0)
    got = (st.centre.cpu().numpy() if centre else None, st.partials.sum(0)[:W].cpu().numpy(), agg.cpu().numpy())
    return got, (s, ((xd - s) ** 2).sum(1))


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
@pytest.mark.parametrize("W", [3, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("centre", [True, False], ids=["cclip", "geomed"])
@pytest.mark.parametrize("kind", ["init", "mid", "last"])
def test_one_pass_bit_for_bit(kind, centre, W, wire):
    (v, d2, agg), (s, want_d2) = _pass(kind, centre, W, wire)
    if centre:
        assert (v == s).all()  # init leaves the centre as it was
    if kind == "last":
        assert (agg[:N] == 0.5 * s).all() and (agg[N:] == -7.0).all()
    else:
        assert (d2 == want_d2).all() and (agg == -7.0).all()


@pytest.mark.parametrize("W", [5, 17])
@pytest.mark.parametrize("centre", [True, False], ids=["cclip", "geomed"])
def test_unaligned_source_and_a_nan_wire_with_zero_weight(centre, W):
    (v, d2, _), (s, want_d2) = _pass("mid", centre, W, "fp16", shift=1)
    (v1, d21, _), _ = _pass("mid", centre, W, "fp16")
    assert (d2 == want_d2).all() and (d2 == d21).all() and (not centre or ((v == s).all() and (v == v1).all()))
    (v, d2, _), (s, want_d2) = _pass("mid", centre, W, "fp16", nan=2)
    keep = np.arange(W) != 2
    assert not np.isfinite(d2[2]) and (d2[keep] == want_d2[keep]).all()
    assert not centre or (np.isfinite(v).all() and (v == s).all())
    (_, _, agg), (s, _) = _pass("last", centre, W, "fp16", nan=2)
    assert (agg[:N] == 0.5 * s).all()


@pytest.mark.parametrize("rule", ["geomed", "cclip"])
def test_weights_kernel_against_fp64(rule):
    tau, nu, W = 2.0, 1e-3, 6
    d2 = np.array([0.0, (nu / 4) ** 2, np.inf, np.nan, (3 * tau) ** 2, (tau / 3) ** 2])
    st = K.RobustIterState(N, "cuda")
    st.partials[1, :W] = torch.from_numpy(d2).cuda()  # the other blocks are zero
    for _ in range(2):
        K.robust_iter_weights(st, W, rule, tau=tau, eps=nu, final=True)
    got = st.read()
    d = np.sqrt(np.where(np.isfinite(d2), d2, np.inf))
    with np.errstate(divide="ignore"):
        w = np.where(np.isinf(d), 0.0, 1.0 / np.maximum(d, nu) if rule == "geomed" else np.minimum(1.0, tau / d) / W)
    a = w / w.sum() if rule == "geomed" else w
    b = 0.0 if rule == "geomed" else 1.0 - a.sum()
    assert (np.abs(np.array(got["a"][:W]) - a) <= 2 * U * a).all() and got["a"][W:] == [0.0] * (32 - W)
    assert np.allclose(got["d"][:W], d, rtol=2.0 ** -51, atol=0)
    assert abs(got["b"] - b) <= 2 * U  # sum |a_k| <= 1, each a_k within 2^-25 of it, then fl(b)
    assert (got["rounds"], got["degenerate_rounds"]) == (2, 0)
    if rule == "geomed":
        assert got["wsum"] == [2.0 * v for v in got["a"]]
    else:
        assert got["clipped"][:W] == [0, 0, 2, 2, 2, 0]


@pytest.mark.parametrize("kind", ["geomed", "cclip"])
def test_combine_on_the_contaminated_round(kind):
    x, honest, r = contaminated()
    W, n = x.shape
    rb = RB.Robust(PSConfig(aggregate=kind, cclip_tau=1.0), n, "cuda")
    srcs, out, v, xd = list(x.cuda()), torch.empty(n, device="cuda"), None, x.double().numpy()
    for _ in range(3 if kind == "cclip" else 1):
        e = rb.combine(srcs, out, 1.0, True).double().cpu().numpy()
        want, a, _ = ref64(xd, kind, 3, 1.0, v=v)
        v = want if kind == "cclip" else None
        # the fp32 combine_host is within 1.052 W u sum_k |a_k g_k| of fp64 on these rounds (measured: geomed 0.382,
        # cclip 0.733 / 1.016 / 1.051); the device sums its distances in another order: 4 x that factor
        bound = 4 * 1.052 * W * U * sum(np.abs(a[k] * xd[k]) for k in range(W) if a[k] != 0.0)
        print(f"{kind}: max err / bound {(np.abs(e - want) / bound).max():.3f}")
        assert (np.abs(e - want) <= bound).all() and np.sqrt(((e - honest) ** 2).sum()) <= r


@pytest.mark.parametrize("kw", [dict(aggregate="geomed"), dict(aggregate="cclip", cclip_tau=0.5)], ids=["geomed", "cclip"])
def test_device_server_matches_cpu_arena(kw):
    cpu, dev = (_server(d, optimizer="sgd", momentum=0.9, **kw) for d in ("cpu", "cuda"))
    gen, rounds = torch.Generator().manual_seed(11), []
    for _ in range(2):
        base = torch.randn(cpu.n, generator=gen) * 1e-2
        rounds.append([(base + torch.randn(cpu.n, generator=gen) * 1e-3).half() for _ in range(5)])
        rounds[-1][3] = rounds[-1][3] * float("nan")
    _drive(cpu, rounds)
    _drive(dev, rounds)
    assert bool(torch.isfinite(dev.params).all())
    assert torch.allclose(cpu.params, dev.params.cpu(), rtol=0, atol=1e-5)
    assert dev.final_metrics()["robust_aggregate"] == cpu.final_metrics()["robust_aggregate"]
