"""The fp64 reference of the SGD server update (csrc/kernels/optim.hip: sgd_apply, sgd_apply_multi)
and the error bound its kernels are held to, with the CPU tests that give the bound its meaning:
every plain fp32 evaluation of the formula stays inside it, every wrong update listed below
leaves it, on the inputs the GPU tests use. ``sgd_reference``, ``sgd_inputs`` and ``within`` are
shared with tests/test_sgd_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

from .test_lars_cpu import f32

U = 2.0 ** -24  # unit roundoff of fp32

LR = 0.1
GSCALES = (1.0, 0.25, 1.0 / 3.0, 1.0 / 7.0)
WDS = (0.0, 5e-4)
MOMENTA = (0.0, 0.9)


def sgd_reference(p, srcs, buf, lr, gscale, momentum, wd, first):
    """One update in float64 from exactly the operands the kernel sees: ``p`` fp32, ``srcs`` the
    list of wires (fp16 or fp32, decoded exactly), ``buf`` the fp32 momentum buffer (None or
    ignored without momentum), the hyper-parameters rounded to fp32 first.

        s = sum_k g_k (list order);  d = s * gscale [+ wd * p]
        v = first ? d : momentum * buf + d      (with momentum; otherwise v = d, buffer untouched)
        p' = p - lr * v

    Returns (p', v or None, bound of p', bound of v or None), all float64, one bound per element.

    The bound, first order in u = 2^-24. An fp32 evaluation rounds
      * the sum of W wires W - 1 times (0 + g_0 is exact)           (W - 1) u on sum_k |g_k|
      * s * gscale once                                              W u        on gscale sum |g|
      * wd * p once, and the add of the two once                     (W + 1) u / 2 u on wd |p|
      * momentum * buf once, and the add once                        (W + 2) u / 3 u / 2 u on momentum |buf|
      * lr * v once                                                  (W + 3) u / 4 u / 3 u
      * the subtraction once                                         u |p'|
    so  |p'_fp32 - p'| <= u (lr ((W + 3) gscale sum |g_k| + 4 wd |p| + 3 momentum |buf|) + |p'|)
    and the buffer's error is within the same inner sum without the outer lr, plus u |v| (its own
    last rounding counted once more, which only loosens it). A fused multiply-add removes
    roundings; a step pre-multiplied on the host (lr * gscale, lr * wd) moves one rounding and
    adds none. Both bounds are doubled for the second-order terms and such reorderings. The terms
    are absolute in the magnitudes of the inputs, so an element whose sum cancels is held to the
    same bound as any other: nothing is masked. With ``first`` the buffer is not an operand and
    its term is left out."""
    lr, gscale, momentum, wd = (f32(x) for x in (lr, gscale, momentum, wd))
    W = len(srcs)
    p = p.double()
    s = torch.zeros_like(p)
    sabs = torch.zeros_like(p)
    for g in srcs:
        s = s + g.double()
        sabs = sabs + g.double().abs()
    d = s * gscale
    inner = (W + 3) * gscale * sabs
    if wd != 0.0:
        d = d + wd * p
        inner = inner + 4 * abs(wd) * p.abs()
    v = vb = None
    if momentum != 0.0 and buf is not None:
        if not first:
            d = momentum * buf.double() + d
            inner = inner + 3 * abs(momentum) * buf.double().abs()
        v = d
        vb = 2 * U * (inner + v.abs())
    p_new = p - lr * d
    pb = 2 * U * (lr * inner + p_new.abs())
    return p_new, v, pb, vb


def within(x, ref, bound):
    """Per element: |x - ref| <= bound (a non-finite x is outside)."""
    return (x.double() - ref).abs() <= bound


def assert_within(x, ref, bound, what=""):
    ok = within(x, ref, bound)
    if not bool(ok.all()):
        err = (x.double() - ref).abs()
        worst = int((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).argmax())
        raise AssertionError((what, "outside the bound:", int((~ok).sum()), "of", ok.numel(), "worst at", worst,
                              float(err[worst]), float(bound[worst])))


def sgd_inputs(n, W=1, seed=0):
    """Weights of order 0.05, a momentum buffer of order 1e-2 and W gradients of order 1e-2 (fp32;
    the fp16 wire is ``g.half()``), mixed signs, every gradient element distinct from its
    neighbours. Cached: the tests share them and leave them unchanged."""
    key = (n, W, seed)
    if key not in sgd_inputs.cache:
        gen = torch.Generator().manual_seed(4321 + 7 * seed + n % 1009)
        p = torch.randn(n, generator=gen) * 0.05
        v = torch.randn(n, generator=gen) * 1e-2
        gs = [torch.randn(n, generator=gen) * 1e-2 for _ in range(W)]
        sgd_inputs.cache[key] = (p, v, gs)
    return sgd_inputs.cache[key]


sgd_inputs.cache = {}


# ---------------------------------------------------------------------------- fp32 evaluations
def _r32(x):
    """float64 -> nearest fp32 (the rounding of a fused multiply-add emulated through float64:
    an fp32 product is exact in float64, the sum rounds once there and once here)."""
    return x.float()


def eval_fp32(p, srcs, buf, lr, gscale, momentum, wd, first, *, premul=False, fused=False):
    """A plain fp32 evaluation of the update. ``premul``: the step multiplied on the host,
    p - ((lr * gscale) * s + (lr * wd) * p), instead of p - lr * (s * gscale + wd * p) (without
    momentum only: with momentum the buffer needs d itself). ``fused``: the final multiply-add
    (and the weight-decay one) as a single rounding."""
    lr32, gs32, mom32, wd32 = (torch.tensor(f32(x), dtype=torch.float32) for x in (lr, gscale, momentum, wd))
    s = torch.zeros_like(p)
    for g in srcs:
        s = s + g.float()
    mom = momentum != 0.0 and buf is not None
    if premul:
        assert not mom
        step, wstep = lr32 * gs32, lr32 * wd32
        if fused and wd:
            return p - _r32(step.double() * s.double() + (wstep * p).double()), None
        if fused:
            return _r32(p.double() - step.double() * s.double()), None
        t = step * s + wstep * p if wd else step * s
        return p - t, None
    d = s * gs32
    if wd:
        d = _r32(wd32.double() * p.double() + d.double()) if fused else d + wd32 * p
    v = None
    if mom:
        if not first:
            d = _r32(mom32.double() * buf.double() + d.double()) if fused else mom32 * buf + d
        v = d
    p_new = _r32(p.double() - lr32.double() * d.double()) if fused else p - lr32 * d
    return p_new, v


N_CPU = 2053
GRID = [(gs, wd, mom, first) for gs, wd, mom in itertools.product(GSCALES, WDS, MOMENTA)
        for first in ((False, True) if mom else (False,))]


def _wires(gs, dtype):
    return [g.to(dtype) for g in gs]


@pytest.mark.parametrize("W", [1, 2, 7, 32])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_fp32_evaluations_stay_inside(W, dtype):
    """Both operation orders, each with and without the fused multiply-add, over the whole grid of
    hyper-parameters, at the sizes the GPU tests use."""
    for n in (1, 7, 8, 9, 255, N_CPU):
        p, buf, gs = sgd_inputs(n, W)
        srcs = _wires(gs, dtype)
        for gscale, wd, mom, first in GRID:
            p_ref, v_ref, pb, vb = sgd_reference(p, srcs, buf, LR, gscale, mom, wd, first)
            assert (v_ref is None) == (mom == 0.0)
            for premul, fused in itertools.product((False, True), (False, True)):
                if premul and mom:
                    continue
                got_p, got_v = eval_fp32(p, srcs, buf, LR, gscale, mom, wd, first, premul=premul, fused=fused)
                what = (n, W, dtype, gscale, wd, mom, first, premul, fused)
                assert_within(got_p, p_ref, pb, what)
                if mom:
                    assert_within(got_v, v_ref, vb, what)


def test_numpy_evaluation_stays_inside():
    """The same formula in numpy fp32 (another implementation of the same arithmetic)."""
    p, buf, gs = sgd_inputs(N_CPU, 7)
    srcs = _wires(gs, torch.float16)
    for gscale, wd, mom, first in GRID:
        p_ref, v_ref, pb, vb = sgd_reference(p, srcs, buf, LR, gscale, mom, wd, first)
        s = np.zeros(N_CPU, np.float32)
        for g in srcs:
            s = s + g.numpy().astype(np.float32)
        d = s * np.float32(gscale)
        if wd:
            d = d + np.float32(wd) * p.numpy()
        if mom and not first:
            d = np.float32(mom) * buf.numpy() + d
        out = p.numpy() - np.float32(LR) * d
        assert out.dtype == np.float32
        assert_within(torch.from_numpy(out), p_ref, pb, (gscale, wd, mom, first))
        if mom:
            assert_within(torch.from_numpy(d), v_ref, vb, (gscale, wd, mom, first))


# ---------------------------------------------------------------------------- wrong updates
def _mutant(name, p, srcs, buf, lr, gscale, mom, wd, first):
    """The update with one mistake, evaluated in float64 (so nothing but the mistake separates it
    from the reference). Returns (p', v) where v is what the buffer holds afterwards."""
    lr, gscale, mom, wd = (f32(x) for x in (lr, gscale, mom, wd))
    pd, bd = p.double(), buf.double()
    use = srcs[:-1] if name == "last_source_skipped" else srcs
    if name == "fp16_sum":
        s16 = torch.zeros(p.numel(), dtype=torch.float16)
        for g in use:
            s16 = s16 + g  # rounds the running sum to fp16 at every step
        s = s16.double()
    else:
        s = torch.zeros_like(pd)
        for g in use:
            s = s + g.double()
    d = s * gscale
    if name == "gscale_twice":
        d = d * gscale
    if wd and name not in ("wd_dropped", "wd_on_new_p"):
        d = d + wd * pd
    v = None
    if mom:
        if name == "momentum_on_d":
            v = d if first else bd + mom * d
        elif name == "first_ignored":
            v = mom * bd + d
        else:
            v = d if first else mom * bd + d
        d = v
        if name == "buffer_not_written":
            v = bd
    p_new = pd - lr * d
    if name == "wd_on_new_p" and wd:
        p_new = p_new - lr * wd * p_new
    return p_new, v


# mutation -> (the hyper-parameter points it applies to, what it must push outside: "p", "v")
MUTATIONS = {
    "wd_dropped": (lambda gs, wd, mom, first, W: wd != 0, "p"),
    "wd_on_new_p": (lambda gs, wd, mom, first, W: wd != 0, "p"),
    "gscale_twice": (lambda gs, wd, mom, first, W: gs != 1, "p"),
    "last_source_skipped": (lambda gs, wd, mom, first, W: True, "p"),
    "fp16_sum": (lambda gs, wd, mom, first, W: W > 1, "p"),
    "first_ignored": (lambda gs, wd, mom, first, W: mom != 0 and first, "p"),
    "buffer_not_written": (lambda gs, wd, mom, first, W: mom != 0, "v"),
    "momentum_on_d": (lambda gs, wd, mom, first, W: mom != 0 and not first, "p"),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("W", [1, 2, 7, 32])
def test_wrong_updates_leave_the_bound(name, W):
    """Each mistake is outside the bound at every hyper-parameter point it applies to, on the
    n = 2053 inputs of the GPU tests (fp16 wires; the momentum mutations also move the buffer)."""
    applies, where = MUTATIONS[name]
    p, buf, gs = sgd_inputs(N_CPU, W)
    srcs = _wires(gs, torch.float16)
    seen = 0
    for gscale, wd, mom, first in GRID:
        if not applies(gscale, wd, mom, first, W):
            continue
        seen += 1
        p_ref, v_ref, pb, vb = sgd_reference(p, srcs, buf, LR, gscale, mom, wd, first)
        got_p, got_v = _mutant(name, p, srcs, buf, LR, gscale, mom, wd, first)
        bad_p = int((~within(got_p, p_ref, pb)).sum())
        bad_v = int((~within(got_v, v_ref, vb)).sum()) if mom else 0
        assert (bad_p if where == "p" else bad_v) > 0, (name, W, gscale, wd, mom, first, bad_p, bad_v)
    assert seen or (name == "fp16_sum" and W == 1)


def test_unmutated_float64_is_inside():
    """The mutation harness without a mutation reproduces the reference (so a mutation's distance
    is the mutation's alone)."""
    p, buf, gs = sgd_inputs(N_CPU, 7)
    srcs = _wires(gs, torch.float16)
    for gscale, wd, mom, first in GRID:
        p_ref, v_ref, pb, vb = sgd_reference(p, srcs, buf, LR, gscale, mom, wd, first)
        got_p, got_v = _mutant("none", p, srcs, buf, LR, gscale, mom, wd, first)
        assert torch.equal(got_p, p_ref) and (not mom or torch.equal(got_v, v_ref))


def test_reference_conventions():
    """fp16 wires are decoded exactly, hyper-parameters are the fp32 values, a NaN buffer is not an
    operand under ``first``, and without momentum there is no buffer result."""
    p, buf, gs = sgd_inputs(255, 2)
    srcs = _wires(gs, torch.float16)
    p_ref, v_ref, pb, vb = sgd_reference(p, srcs, torch.full_like(buf, float("nan")), LR, 1 / 3, 0.9, 5e-4, True)
    assert bool(torch.isfinite(p_ref).all() and torch.isfinite(v_ref).all() and torch.isfinite(pb).all())
    want = p.double() - f32(LR) * ((srcs[0].double() + srcs[1].double()) * f32(1 / 3) + f32(5e-4) * p.double())
    assert torch.equal(p_ref, want)
    assert sgd_reference(p, srcs, buf, LR, 1.0, 0.0, 0.0, False)[1] is None
    assert bool((pb > 0).all()) and float((pb / p_ref.abs().clamp_min(1e-3)).max()) < 1e-5
