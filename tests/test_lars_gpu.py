"""The LARS update kernels (csrc/kernels/lars.hip) on a synthetic layout against the fp64
reference of tests/test_lars_cpu.py: trust ratios, update, momentum buffer, bf16 image, the
excluded 1-D tensor against sgd_apply_multi, reproducibility, guard bands, and the segment table
of the real ResNet-18 layout."""
import pytest
import torch

from psx.models.layout import Entry, ParamLayout
from psx.ops import kernels as K

from .test_lars_cpu import assert_buf_close, assert_update_close, lars_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
CH = K.LARS_CHUNK
LR, TRUST, EPS = 0.1, 0.001, 1e-8


def make_layout(sizes) -> ParamLayout:
    """Tensors packed back to back: (name, numel, ndim); 2-D ones are (numel, 1)."""
    lay = ParamLayout()
    off = 0
    for name, numel, ndim in sizes:
        shape = (numel, 1) if ndim > 1 else (numel,)
        lay.entries[name] = Entry(name, shape, "float32", "param", off, numel)
        off += numel
    lay.param_numel = off
    return lay


# sizes 1, 7, 255, chunk-1, chunk, chunk+1, 3 chunk+5 (later tensors start at odd offsets), a 1-D
# tensor (excluded from adaptation), an all-zero gradient and all-zero weights (ratio 1 each)
SIZES = [("t1", 1, 2), ("t7", 7, 2), ("t255", 255, 2), ("tcm1", CH - 1, 2), ("tc", CH, 2), ("tcp1", CH + 1, 2),
         ("t3c5", 3 * CH + 5, 2), ("bias", 100, 1), ("zerograd", 513, 2), ("zerow", 129, 2)]
LAYOUT = make_layout(SIZES)
N = LAYOUT.param_numel

VARIANTS = {"plain": dict(momentum=0.0, wd=0.0, first=False), "mom_first": dict(momentum=0.9, wd=0.0, first=True),
            "mom": dict(momentum=0.9, wd=0.0, first=False), "wd": dict(momentum=0.0, wd=5e-4, first=False),
            "mom_wd": dict(momentum=0.9, wd=5e-4, first=False)}


def _layout_key(layout):
    return tuple((e.name, e.numel) for e in layout.entries.values())


def _inputs(layout=LAYOUT, seed=0):
    """CPU inputs, built once per layout: weights, momentum buffer and 7 gradients. Every element
    has one sign shared by its weight, its buffer value and its gradients: the bounds checked here
    are relative to the result, which g + wd * w and momentum * v + d meet only where they do not
    cancel (signs differ from element to element, and the norms do not see them)."""
    key = (_layout_key(layout), seed)
    if key not in _inputs.cache:
        n = layout.param_numel
        gen = torch.Generator().manual_seed(1234 + seed)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        p = sign * (torch.randn(n, generator=gen).abs() * 0.05 + 1e-3)
        v = sign * torch.randn(n, generator=gen).abs() * 1e-2
        gs = [sign * torch.randn(n, generator=gen).abs() * 1e-2 for _ in range(7)]
        for name in ("zerograd", "zerow"):
            if name in layout.entries:
                e = layout.entries[name]
                for t in (gs if name == "zerograd" else [p]):
                    t[e.offset:e.offset + e.numel] = 0
        _inputs.cache[key] = (p, v, gs)
    return _inputs.cache[key]


_inputs.cache = {}


def _sum_fp32(srcs):
    """The fp32 sum of the decoded sources in source order, as sgd_apply_multi forms it."""
    s = torch.zeros_like(srcs[0], dtype=torch.float32)
    for g in srcs:
        s = s + g.float()
    return s


def _banded(x: torch.Tensor, pad: int, fill: float):
    """x on the device inside an allocation with ``pad`` guard elements on either side."""
    big = torch.full((pad + x.numel() + pad,), fill, dtype=x.dtype, device=DEV)
    big[pad:pad + x.numel()] = x.to(DEV)
    return big, big[pad:pad + x.numel()]


def _guards_intact(big: torch.Tensor, pad: int, fill: float) -> bool:
    ref = torch.full((pad,), fill, dtype=big.dtype, device=DEV)
    return torch.equal(big[:pad], ref) and torch.equal(big[-pad:], ref)


def _reference(layout, W, dtype, variant, seed=0):
    key = (_layout_key(layout), W, dtype, variant, seed)
    if key not in _reference.cache:
        p, v, gs = _inputs(layout, seed)
        s = _sum_fp32([g.to(dtype) for g in gs[:W]])
        kw = VARIANTS[variant]
        _reference.cache[key] = (s,) + lars_reference(layout, p, s, v, lr=LR, gscale=1.0 / W, trust=TRUST, eps=EPS,
                                                      f32_hparams=True, **kw)
    return _reference.cache[key]


_reference.cache = {}


def _run(table, W, dtype, variant, pad, img_on, dense=False, layout=LAYOUT):
    """One update on guarded device buffers. Returns the device views and the guard check."""
    p, v, gs = _inputs(layout)
    n = layout.param_numel
    kw = VARIANTS[variant]
    bufs = {"p": _banded(p, pad, 7.0), "stage": _banded(torch.zeros(n), pad, 9.0)}
    if kw["momentum"]:
        bufs["buf"] = _banded(v, pad, 5.0)
    if img_on:
        bufs["img"] = _banded(torch.zeros(n, dtype=torch.bfloat16), pad, 3.0)
    srcs = [_banded(g.to(dtype), pad, 1.0) for g in gs[:W]]
    args = dict(lr=LR, gscale=1.0 / W, trust=TRUST, eps=EPS, buf=bufs["buf"][1] if "buf" in bufs else None,
                img=bufs["img"][1] if img_on else None, **kw)
    if dense:
        s = srcs[0][1].float().clone()  # chained fp32 adds in source order
        for big, view in srcs[1:]:
            s += view.float()
        bufs["stage"][1].copy_(s)
        K.lars_apply(bufs["p"][1], bufs["stage"][1], table, **args)
    else:
        K.lars_apply_multi(bufs["p"][1], [view for _, view in srcs], bufs["stage"][1], table, **args)
    torch.cuda.synchronize()
    fills = {"p": 7.0, "stage": 9.0, "buf": 5.0, "img": 3.0}
    intact = all(_guards_intact(big, pad, fills[k]) for k, (big, _) in bufs.items())
    intact = intact and all(_guards_intact(big, pad, 1.0) for big, _ in srcs)
    src_same = all(torch.equal(view.cpu(), g.to(dtype)) for (_, view), g in zip(srcs, gs))
    return {k: view for k, (_, view) in bufs.items()}, intact and src_same


@pytest.fixture(scope="module")
def table():
    return K.lars_table(LAYOUT, DEV)


@pytest.mark.parametrize("pad", [64, 3])  # 16-byte aligned views (vector body) / element-aligned (scalar)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("W", [1, 3, 7])
def test_update_matches_reference(table, W, dtype, variant, pad):
    """Ratios within 1e-5 relative (the chunk gives a lane at most 8192 / 256 + 2 = 34 fp32 terms,
    below the 64 the bound was derived for), update and momentum buffer within the issue's bounds,
    image bit-equal to the bf16 of the new parameters, staged sum equal to the fp32 source-order
    sum, the 1-D tensor bit-equal to sgd_apply_multi with wd = 0, nothing written outside
    [0, n); with and without the image."""
    p_old, v_old, gs = _inputs()
    s_ref, p_ref, v_ref, ratios = _reference(LAYOUT, W, dtype, variant)
    kw = VARIANTS[variant]
    outs = []
    for img_on in (False, True):
        out, intact = _run(table, W, dtype, variant, pad, img_on)
        assert intact, "guard bands / sources"
        assert torch.equal(out["stage"].cpu(), s_ref)
        lam = table.ratios.cpu().double()
        want = torch.tensor([ratios[nm] for nm in table.names], dtype=torch.float64)
        assert bool(((lam - want).abs() <= 1e-5 * want.abs()).all()), (lam, want)
        for nm in ("bias", "zerograd", "zerow"):
            assert float(lam[table.names.index(nm)]) == 1.0
        assert_update_close(out["p"].cpu(), p_old, p_ref, (W, dtype, variant, pad))
        if kw["momentum"]:
            assert_buf_close(out["buf"].cpu(), v_ref, (W, dtype, variant, pad))
        if img_on:
            assert torch.equal(out["img"], out["p"].bfloat16())
        outs.append(out)
    assert torch.equal(outs[0]["p"], outs[1]["p"])  # the image does not change the update
    # the excluded 1-D tensor: the SGD kernel on the same slice, no weight decay
    e = LAYOUT.entries["bias"]
    sl = slice(e.offset, e.offset + e.numel)
    ps = p_old[sl].to(DEV)
    bs = v_old[sl].to(DEV) if kw["momentum"] else None
    K.sgd_apply_multi(ps, [g.to(dtype)[sl].to(DEV) for g in gs[:W]], LR, gscale=1.0 / W, momentum=kw["momentum"],
                      wd=0.0, buf=bs, first=kw["first"])
    assert torch.equal(outs[0]["p"][sl].view(torch.int32), ps.view(torch.int32))
    if bs is not None:
        assert torch.equal(outs[0]["buf"][sl].view(torch.int32), bs.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("W", [1, 3, 7])
def test_reproducible_and_dense_entry(table, W, dtype):
    """Two runs on identical inputs are bit-identical, and the dense entry (the sum formed by
    chained fp32 adds in source order) ends in the same bits as the multi-source entry, with
    aligned and with element-aligned buffers."""
    runs = []
    for pad, dense in ((64, False), (64, False), (64, True), (3, False), (3, True)):
        out, intact = _run(table, W, dtype, "mom_wd", pad, True, dense=dense)
        assert intact
        runs.append((out, table.ratios.clone()))
    (a, ra) = runs[0]
    for b, rb in runs[1:]:
        assert torch.equal(ra, rb)
        for k in ("p", "buf", "img", "stage"):
            assert torch.equal(a[k], b[k]), k


def test_many_partials():
    """A tensor of more than 256 chunks (the apply sums a tensor's partials 256 at a time) after
    a short one, so its chunks start at an odd offset."""
    lay = make_layout([("t7", 7, 2), ("big", 300 * CH + 17, 2), ("bias", 100, 1)])
    tab = K.lars_table(lay, DEV)
    assert tab.nblocks == 1 + 301 + 1
    p_old, v_old, _ = _inputs(lay)
    s_ref, p_ref, v_ref, ratios = _reference(lay, 2, torch.float16, "mom_wd")
    out, intact = _run(tab, 2, torch.float16, "mom_wd", 64, True, layout=lay)
    assert intact and torch.equal(out["stage"].cpu(), s_ref)
    lam = tab.ratios.cpu().double()
    want = torch.tensor([ratios[nm] for nm in tab.names], dtype=torch.float64)
    assert bool(((lam - want).abs() <= 1e-5 * want.abs()).all()), (lam, want)
    assert_update_close(out["p"].cpu(), p_old, p_ref)
    assert_buf_close(out["buf"].cpu(), v_ref)
    assert torch.equal(out["img"], out["p"].bfloat16())


def test_capturable(table):
    """Both launches go on the caller's stream without a host synchronisation: the update can be
    captured into a HIP graph, and a replay gives the bits of the eager update."""
    p_old, v_old, gs = _inputs()
    srcs = [g.half().to(DEV) for g in gs[:3]]
    kw = dict(lr=LR, gscale=1 / 3, momentum=0.9, wd=5e-4, trust=TRUST, eps=EPS, first=False)
    res = []
    for graph in (False, True):
        p, v, stage = p_old.to(DEV), v_old.to(DEV), torch.zeros(N, device=DEV)
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                K.lars_apply_multi(p, srcs, stage, table, buf=v, **kw)
            p.copy_(p_old)
            v.copy_(v_old)
            g.replay()
        else:
            K.lars_apply_multi(p, srcs, stage, table, buf=v, **kw)
        torch.cuda.synchronize()
        res.append((p.clone(), v.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_argument_checks(table):
    p = torch.zeros(N, device=DEV)
    stage = torch.zeros(N, device=DEV)
    with pytest.raises(AssertionError):
        K.lars_apply_multi(p, [stage], stage, table, LR)  # a source aliasing the staging buffer
    with pytest.raises(AssertionError):
        K.lars_apply_multi(p[:-1], [torch.zeros(N, device=DEV)], stage, table, LR)
    with pytest.raises(AssertionError):
        K.lars_apply(p, stage.half(), table, LR)
    with pytest.raises(AssertionError):
        K.lars_apply_multi(p, [torch.zeros(N, device=DEV)] * 33, stage, table, LR)


def test_table_round_trips_resnet18():
    from psx.models.resnet import build_model

    lay = ParamLayout.from_module(build_model("resnet18", 100))
    tab = K.lars_table(lay, DEV)
    rec = tab.records()
    summ = lay.summary()
    assert len(rec) == tab.ntensors == summ["trainable_tensors"]
    assert int(rec["numel"].sum()) == summ["trainable_params"] == tab.n
    ents = [e for e in lay.entries.values() if e.region == "param"]
    assert [int(o) for o in rec["offset"]] == [e.offset for e in ents]
    assert [int(x) for x in rec["numel"]] == [e.numel for e in ents]
    assert [bool(a) for a in rec["adapt"]] == [len(e.shape) > 1 for e in ents]
    fb = [int(x) for x in rec["first_block"]]
    assert fb[0] == 0 and all(b > a for a, b in zip(fb, fb[1:]))
    assert [b - a for a, b in zip(fb, fb[1:] + [tab.nblocks])] == [-(-e.numel // CH) for e in ents]
    assert tab.partials.numel() == 2 * tab.nblocks and tab.ratios.numel() == tab.ntensors
    assert K.kernels().psx_lars_table_size() == rec.dtype.itemsize == 24
    assert K.kernels().psx_lars_chunk() == CH


def test_server_paths_agree():
    """ParameterServer on the device: the fp16 wire (multi-source entry), a q8 payload and a top-k
    payload (decoded into the aggregation buffer, dense entry) against the fp64 reference on the
    decoded gradient, two pushes each; the ratio summary of final_metrics comes from the table."""
    from psx.models.resnet import TinyResNet
    from psx.parallel import q8 as Q
    from psx.parallel import topk as T
    from psx.parallel.server import ParameterServer

    from .test_ps_cpu import tiny_cfg

    for kind in ("fp16", "q8", "topk"):
        torch.manual_seed(2)
        m = TinyResNet(10)
        lay = ParamLayout.from_module(m)
        arena, counters = lay.pack(m)
        n = lay.param_numel
        cfg = tiny_cfg(mode="async", workers=1, optimizer="lars", codec=kind, momentum=0.9, weight_decay=5e-4, lr=0.1,
                       topk_ratio=0.25)
        s = ParameterServer(cfg, lay, arena.clone(), counters, device=DEV, total_workers=1, log=lambda *a: None)
        s.register_worker("w", 0)
        sign = torch.where(s.params >= 0, 1.0, -1.0).cpu()
        gen = torch.Generator().manual_seed(11)
        enc = Q.Q8Codec(n, DEV) if kind == "q8" else T.TopKCodec(n, cfg.topk_ratio, DEV) if kind == "topk" else None
        for step in range(2):
            g = (sign * torch.randn(n, generator=gen).abs() * 1e-2).to(DEV)
            if kind == "fp16":
                wire = g.half()
                dense = wire.float()
            else:
                enc.resid.zero_()
                wire = enc.encode(g).clone()
                dense = (Q.decode(wire, n) if kind == "q8" else
                         T.decode_add(wire, torch.zeros(n, device=DEV), 1.0, T.topk_k(n, cfg.topk_ratio))).clone()
            p_old, v_old = s.params.cpu(), s.momentum_buf.cpu()
            p_ref, v_ref, ratios = lars_reference(lay, p_old, dense.cpu(), v_old, lr=cfg.lr, gscale=1.0,
                                                  momentum=cfg.momentum, wd=cfg.weight_decay, trust=cfg.lars_trust,
                                                  eps=cfg.lars_eps, first=step == 0, f32_hparams=True)
            s.apply(wire, 1.0)
            assert_update_close(s.params.cpu(), p_old, p_ref, (kind, step))
            assert_buf_close(s.momentum_buf.cpu(), v_ref, (kind, step))
        adapted = torch.tensor([ratios[e.name] for e in lay.entries.values()
                                if e.region == "param" and len(e.shape) > 1])
        got = s.final_metrics()["lars_trust_ratio"]
        for key, want in (("min", adapted.min()), ("median", adapted.median()), ("max", adapted.max())):
            assert got[key] == pytest.approx(float(want), rel=1e-5)


def test_server_weight_image():
    """With the weight-image fetch path on, the LARS apply writes the bf16 image of the updated
    parameters in the same pass (no stale wire)."""
    from psx.models.resnet import TinyResNet
    from psx.parallel.server import ParameterServer

    from .test_ps_cpu import tiny_cfg

    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    n = lay.param_numel
    cfg = tiny_cfg(mode="async", workers=1, optimizer="lars", momentum=0.9, weight_decay=5e-4, lr=0.1, dtype="bf16")
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=DEV, total_workers=1, log=lambda *a: None)
    s.register_worker("w", 0)
    s.enable_weight_wire()
    before = s.params.clone()
    s.apply((torch.randn(n, generator=torch.Generator().manual_seed(3)) * 1e-2).half().to(DEV), 1.0)
    assert not s._wire_stale and not torch.equal(before, s.params)
    assert torch.equal(s.wire.img[:n], s.params.bfloat16())
