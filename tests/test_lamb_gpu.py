"""The LAMB update kernels (csrc/kernels/lamb.hip) on the synthetic layout of the LARS kernel
tests against the fp64 reference of tests/test_lamb_cpu.py: moments bit-equal to the AdamW
kernel's, ratios, the update u in the staging buffer, p' as one fma of the device's own u and
ratio, every form (multi-source / dense entry, aligned / element-aligned, image on / off) in the
same bits, reproducibility, guard bands, the C ABI's refusals and the segment table of the real
ResNet-18 layout."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.ops import kernels as K

from .test_lamb_cpu import assert_lamb_close, f32, fma32, lamb_reference
from .test_lars_gpu import CH, DEV, LAYOUT, N, _banded, _guards_intact, _sum_fp32, make_layout

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 2e-3, 0.9, 0.999, 1e-8
FILLS = {"p": 7.0, "stage": 9.0, "m": 5.0, "v": 4.0, "img": 3.0}


def _layout_key(layout):
    return tuple((e.name, e.numel) for e in layout.entries.values())


def _inputs(layout=LAYOUT):
    """CPU inputs, built once per layout: weights, both moments and 7 gradients, signs at random
    (the bounds are relative to magnitude sums). The all-zero-gradient tensor also has zero
    moments (u = wd * w: both norm rules are met with wd = 0), the all-zero-weight tensor w = 0."""
    key = _layout_key(layout)
    if key not in _inputs.cache:
        n = layout.param_numel
        gen = torch.Generator().manual_seed(4321)
        p = torch.randn(n, generator=gen) * 0.05
        m = torch.randn(n, generator=gen) * 5e-3
        v = torch.randn(n, generator=gen).square() * 1e-4
        gs = [torch.randn(n, generator=gen) * 1e-2 for _ in range(7)]
        for name in ("zerograd", "zerow"):
            if name in layout.entries:
                e = layout.entries[name]
                for t in (gs + [m, v] if name == "zerograd" else [p]):
                    t[e.offset:e.offset + e.numel] = 0
        _inputs.cache[key] = (p, m, v, gs)
    return _inputs.cache[key]


_inputs.cache = {}


def _scalars(t):
    return K.lamb_scalars(t, beta1=B1, beta2=B2, eps=EPS)


def _reference(layout, W, dtype, t, wd):
    key = (_layout_key(layout), W, dtype, t, wd)
    if key not in _reference.cache:
        p, m, v, gs = _inputs(layout)
        s = _sum_fp32([g.to(dtype) for g in gs[:W]])
        _reference.cache[key] = (s, lamb_reference(layout, p, m, v, s, _scalars(t), f32(1.0 / W), f32(wd)))
    return _reference.cache[key]


_reference.cache = {}


def _run(table, W, dtype, t, wd, pad=64, img_on=False, dense=False, layout=LAYOUT):
    """One update on guarded device buffers. Returns the device views, the ratios and whether the
    guard bands and the sources are intact."""
    p, m, v, gs = _inputs(layout)
    n = layout.param_numel
    bufs = {"p": _banded(p, pad, FILLS["p"]), "stage": _banded(torch.zeros(n), pad, FILLS["stage"]),
            "m": _banded(m, pad, FILLS["m"]), "v": _banded(v, pad, FILLS["v"])}
    if img_on:
        bufs["img"] = _banded(torch.zeros(n, dtype=torch.bfloat16), pad, FILLS["img"])
    srcs = [_banded(g.to(dtype), pad, 1.0) for g in gs[:W]]
    args = dict(lr=LR, t=t, gscale=1.0 / W, wd=wd, beta1=B1, beta2=B2, eps=EPS,
                img=bufs["img"][1] if img_on else None)
    if dense:
        s = srcs[0][1].float().clone()  # chained fp32 adds in source order
        for _, view in srcs[1:]:
            s += view.float()
        bufs["stage"][1].copy_(s)
        K.lamb_apply(bufs["p"][1], bufs["stage"][1], bufs["m"][1], bufs["v"][1], table, **args)
    else:
        K.lamb_apply_multi(bufs["p"][1], [view for _, view in srcs], bufs["stage"][1], bufs["m"][1], bufs["v"][1],
                           table, **args)
    torch.cuda.synchronize()
    intact = all(_guards_intact(big, pad, FILLS[k]) for k, (big, _) in bufs.items())
    intact = intact and all(_guards_intact(big, pad, 1.0) for big, _ in srcs)
    src_same = all(torch.equal(view.cpu(), g.to(dtype)) for (_, view), g in zip(srcs, gs))
    out = {k: view for k, (_, view) in bufs.items()}
    out["ratios"] = table.ratios.clone()
    return out, intact and src_same


def _step_of(table, layout, ratios):
    """fp32 lr * phi of every element, from the device's own ratio table."""
    step = torch.empty(layout.param_numel, dtype=torch.float32)
    lr = np.float32(LR)
    for nm, phi in zip(table.names, ratios.cpu().numpy()):
        e = layout.entries[nm]
        step[e.offset:e.offset + e.numel] = float(lr * np.float32(phi))
    return step


def _check_against_reference(table, layout, out, W, dtype, t, wd, what):
    """Everything the issue asserts of one run; returns the worst error / bound of u."""
    p_old, m_old, v_old, gs = _inputs(layout)
    s_ref, ref = _reference(layout, W, dtype, t, wd)
    # the moments: the AdamW kernel's, bit for bit (its lr and wd touch p only)
    pa, ma, va = p_old.to(DEV), m_old.to(DEV), v_old.to(DEV)
    K.adamw_apply_multi(pa, [g.to(dtype).to(DEV) for g in gs[:W]], ma, va, LR, t, gscale=1.0 / W, beta1=B1, beta2=B2,
                        eps=EPS, wd=0.0)
    assert torch.equal(out["m"].view(torch.int32), ma.view(torch.int32)), what
    assert torch.equal(out["v"].view(torch.int32), va.view(torch.int32)), what
    worst = assert_lamb_close(out["stage"], out["m"], out["v"], ref, what)
    lam = out["ratios"].cpu().double()
    want = torch.tensor([ref["phi"][nm] for nm in table.names], dtype=torch.float64)
    assert bool(((lam - want).abs() <= 1e-5 * want.abs()).all()), (what, lam, want)
    for nm in ("bias", "zerow"):
        if nm in table.names:
            assert float(lam[table.names.index(nm)]) == 1.0
    if "zerograd" in table.names and wd == 0.0:
        assert float(lam[table.names.index("zerograd")]) == 1.0
    # p' = fma(-(lr * phi), u, p) of the device's own u and ratio, bit for bit
    want_p = fma32(out["stage"].cpu(), -_step_of(table, layout, out["ratios"]), p_old)
    assert torch.equal(out["p"].cpu().view(torch.int32), want_p.view(torch.int32)), what
    return worst


@pytest.fixture(scope="module")
def table():
    return K.lars_table(LAYOUT, DEV)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("W", [1, 3, 7])
def test_update_matches_reference(table, W, dtype, t, wd):
    """m', v' bit-equal to adamw_apply_multi's and within adamw_reference's bounds; ratios within
    1e-5 relative; u within 12 U bc1 M / den + k U (|r| + wd |w|) (lamb_reference's docstring:
    no margin over the derivation); p' the one fma of the device's u and ratio; multi-source and
    dense entry, aligned and element-aligned buffers, image on and off, and a second run on the
    same inputs all end in the same bits; the image is the bf16 of p'; nothing is written outside
    [0, n) and the sources stay."""
    what = (W, dtype, t, wd)
    base, intact = _run(table, W, dtype, t, wd)
    assert intact, "guard bands / sources"
    worst = _check_against_reference(table, LAYOUT, base, W, dtype, t, wd, what)
    print(f"lamb u worst error / bound {what}: {worst:.3f}")
    for pad, dense, img_on in itertools.product((64, 3), (False, True), (False, True)):
        out, intact = _run(table, W, dtype, t, wd, pad=pad, img_on=img_on, dense=dense)
        assert intact, (what, pad, dense, img_on)
        for k in ("p", "m", "v", "stage", "ratios"):
            assert torch.equal(out[k].view(torch.int32), base[k].view(torch.int32)), (what, pad, dense, img_on, k)
        if img_on:
            assert torch.equal(out["img"], out["p"].bfloat16())


def test_many_partials():
    """A tensor of more than 256 chunks (the apply sums a tensor's partials 256 at a time) after
    a short one, so its chunks start at an odd offset."""
    lay = make_layout([("t7", 7, 2), ("big", 300 * CH + 17, 2), ("bias", 100, 1)])
    tab = K.lars_table(lay, DEV)
    assert tab.nblocks == 1 + 301 + 1
    out, intact = _run(tab, 2, torch.float16, 3, 1e-2, img_on=True, layout=lay)
    assert intact
    _check_against_reference(tab, lay, out, 2, torch.float16, 3, 1e-2, "many")
    assert torch.equal(out["img"], out["p"].bfloat16())


def test_capturable(table):
    """Both launches go on the caller's stream without a host synchronisation: the update can be
    captured into a HIP graph, and a replay gives the bits of the eager update."""
    p_old, m_old, v_old, gs = _inputs()
    srcs = [g.half().to(DEV) for g in gs[:3]]
    kw = dict(lr=LR, t=2, gscale=1 / 3, wd=1e-2, beta1=B1, beta2=B2, eps=EPS)
    res = []
    for graph in (False, True):
        p, m, v, stage = p_old.to(DEV), m_old.to(DEV), v_old.to(DEV), torch.zeros(N, device=DEV)
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                K.lamb_apply_multi(p, srcs, stage, m, v, table, **kw)
            for dst, src in ((p, p_old), (m, m_old), (v, v_old)):
                dst.copy_(src)
            g.replay()
        else:
            K.lamb_apply_multi(p, srcs, stage, m, v, table, **kw)
        torch.cuda.synchronize()
        res.append((p.clone(), m.clone(), v.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_wrapper_argument_checks(table):
    p, stage, m, v = (torch.zeros(N, device=DEV) for _ in range(4))
    g = torch.zeros(N, device=DEV)
    with pytest.raises(AssertionError):
        K.lamb_apply_multi(p, [stage], stage, m, v, table, LR, 1)  # a source aliasing the staging buffer
    with pytest.raises(AssertionError):
        K.lamb_apply_multi(p, [m], stage, m, v, table, LR, 1)
    with pytest.raises(AssertionError):
        K.lamb_apply_multi(p[:-1], [g], stage, m, v, table, LR, 1)
    with pytest.raises(AssertionError):
        K.lamb_apply(p, stage.half(), m, v, table, LR, 1)
    with pytest.raises(AssertionError):
        K.lamb_apply_multi(p, [g] * 33, stage, m, v, table, LR, 1)
    with pytest.raises(AssertionError):
        K.lamb_apply(p, stage, m, v, table, LR, 0)


def test_c_abi_refusals(table):
    """Every refused argument returns an error and writes nothing."""
    lib = K.kernels()
    gen = torch.Generator().manual_seed(9)
    bufs = {k: torch.randn(N, generator=gen).to(DEV) for k in ("p", "stage", "m", "v", "g")}
    bufs["v"].abs_()
    keep = {k: x.clone() for k, x in bufs.items()}
    ratios0, partials0 = table.ratios.clone(), table.partials.clone()
    P = {k: x.data_ptr() for k, x in bufs.items()}
    st = K.stream_ptr()

    def multi(p="p", srcs=("g",), nsrc=None, stage="stage", m="m", v="v", n=N, t=1, arr=True):
        ptrs = [P[s] if isinstance(s, str) else s for s in srcs]
        a = (C.c_void_p * max(1, len(ptrs)))(*ptrs) if arr else None
        return lib.psx_lamb_apply_multi(P.get(p), a, len(ptrs) if nsrc is None else nsrc, 0, P.get(stage), P.get(m),
                                        P.get(v), n, table.dev.data_ptr(), table.ntensors, table.nblocks,
                                        table.partials.data_ptr(), table.ratios.data_ptr(), LR, 1.0, 0.0, B1, B2, EPS,
                                        t, None, st)

    def dense(p="p", stage="stage", m="m", v="v", n=N, t=1):
        return lib.psx_lamb_apply(P.get(p), P.get(stage), P.get(m), P.get(v), n, table.dev.data_ptr(),
                                  table.ntensors, table.nblocks, table.partials.data_ptr(), table.ratios.data_ptr(),
                                  LR, 1.0, 0.0, B1, B2, EPS, t, None, st)

    bad = [multi(p=None), multi(stage=None), multi(m=None), multi(v=None), multi(arr=False), multi(srcs=(None,)),
           multi(srcs=(), nsrc=0), multi(srcs=("g",) * 33), multi(n=0), multi(n=-5), multi(t=0),
           multi(srcs=("stage",)),  # a source equal to the staging buffer
           multi(srcs=("p",)), multi(srcs=("m",)), multi(srcs=("v",)),
           multi(srcs=(P["p"] + 4 * (N - 1),)),  # overlapping p by one element
           multi(srcs=(P["m"] + 4 * (N - 1),)), multi(srcs=(P["v"] + 4 * (N - 1),)),
           dense(p=None), dense(stage=None), dense(m=None), dense(v=None), dense(n=0), dense(t=0)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    for k, x in bufs.items():
        assert torch.equal(x, keep[k]), k
    assert torch.equal(table.ratios, ratios0) and torch.equal(table.partials, partials0)
    assert multi() == 0  # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not torch.equal(bufs["p"], keep["p"]) and torch.equal(bufs["g"], keep["g"])


def test_table_covers_resnet18():
    from psx.models.resnet import build_model

    lay = ParamLayout.from_module(build_model("resnet18", 100))
    tab = K.lars_table(lay, DEV)
    rec = tab.records()
    off, num = [int(x) for x in rec["offset"]], [int(x) for x in rec["numel"]]
    assert off[0] == 0 and all(o + k == o2 for o, k, o2 in zip(off, num, off[1:])) and off[-1] + num[-1] == tab.n
    assert tab.n == lay.param_numel
    fb = [int(x) for x in rec["first_block"]]
    assert [b - a for a, b in zip(fb, fb[1:] + [tab.nblocks])] == [-(-k // CH) for k in num]
