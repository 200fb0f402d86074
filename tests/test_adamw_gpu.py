"""The AdamW update kernel (csrc/kernels/adamw.hip) against the fp64 reference and bounds of
tests/test_adamw_cpu.py: sizes around the 8-element group and the capped grid, 1..7 fp16 / fp32
sources, bias-correction steps, decay, bf16 image, the three buffer phases (vector body without
and with head, element-wise form) and the one-source dense entry bit-identical to each other,
reproducibility, guard bands, graph capture, argument checks, and ParameterServer on the device."""
import ctypes as C

import pytest
import torch

from psx.ops import kernels as K

from .test_adamw_cpu import _tiny_server, adamw_reference, assert_adamw_close, server_scalars, wires

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
PAD = 128  # guard elements either side of every view (the views start 1..64 elements into them)
# (offset of p, m, v, img; offset of the sources) inside their allocations, in elements:
#   aligned: every view 16-byte aligned, vector body without head
#   shared : one element phase (3) everywhere, head 5, then the vector body
#   mixed  : p, m, v, img at 3 and the sources at 1, no common head: the element-wise form
PHASES = {"aligned": (64, 64), "shared": (3, 3), "mixed": (3, 1)}
# the launch caps its grid at 4096 workgroups of 256 lanes of 8 elements (optim.hip's cap): this n
# sends the grid-stride loop of the vector body on a second trip (and the element-wise form's on
# its ninth)
N_BIG = 8 * 4096 * 256 + 8 * 300 + 3
SIZES = [1, 7, 8, 9, 255, 2048, 3 * 2048 + 5]
FILL = {"p": 7.0, "m": 5.0, "v": 9.0, "img": 3.0, "src": 1.0}

WORST = {"m": 0.0, "v": 0.0, "p": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nadamw kernel: worst error / bound over this module  m %.3f  v %.3f  p %.3f"
          % (WORST["m"], WORST["v"], WORST["p"]))


def _note(worst):
    for k, w in zip(("m", "v", "p"), worst):
        WORST[k] = max(WORST[k], w)


def _inputs(n):
    """CPU inputs, built once per n: weights, moments (v >= 0) and 7 gradients with random
    signs; for n >= 2048 a block with s = m = v = 0 and a block with p = 0."""
    if n not in _inputs.cache:
        gen = torch.Generator().manual_seed(4321 + n % 1000)
        p = torch.randn(n, generator=gen) * 0.05
        m = torch.randn(n, generator=gen) * 1e-2
        v = torch.randn(n, generator=gen).square() * 1e-4
        gs = [torch.randn(n, generator=gen) * 1e-2 for _ in range(7)]
        if n >= 2048:
            for t in gs + [m, v]:
                t[:513] = 0
            p[600:729] = 0
        _inputs.cache[n] = (p, m, v, gs)
    return _inputs.cache[n]


_inputs.cache = {}


def _sum_fp32(srcs):
    """The fp32 sum of the decoded sources in source order, as sgd_apply_multi forms it."""
    s = torch.zeros_like(srcs[0], dtype=torch.float32)
    for g in srcs:
        s = s + g.float()
    return s


class Banded:
    """A view of n elements starting ``off`` elements into a device allocation filled with ``fill``."""

    def __init__(self, n, off, fill, dtype=torch.float32):
        assert 0 < off <= PAD
        self.big = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=DEV)
        self.view, self.off, self.n, self.fill = self.big[off:off + n], off, n, fill

    def intact(self) -> bool:
        lo, hi = self.big[:self.off], self.big[self.off + self.n:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


class Rig:
    """Guarded device buffers of one (n, source dtype, phase): the sources are uploaded once, p, m,
    v are reset before every update."""

    def __init__(self, n, dtype, phase, nsrc=7):
        self.n, self.dtype = n, dtype
        po, so = PHASES[phase]
        self.cpu = _inputs(n)
        self.dev = [x.to(DEV) for x in self.cpu[:3]]
        self.p, self.m, self.v = (Banded(n, po, FILL[k]) for k in "pmv")
        self.img = Banded(n, po, FILL["img"], torch.bfloat16)
        self.srcs = [Banded(n, so, FILL["src"], dtype) for _ in range(nsrc)]
        for b, g in zip(self.srcs, self.cpu[3]):
            b.view.copy_(g.to(dtype))
        self.dense = Banded(n, so, FILL["src"])

    def run(self, W, t, wd, img_on, dense=False):
        for b, x in zip((self.p, self.m, self.v), self.dev):
            b.view.copy_(x)
        kw = dict(gscale=1.0 / W, beta1=B1, beta2=B2, eps=EPS, wd=wd, img=self.img.view if img_on else None)
        if dense:  # chained fp32 adds in source order
            s = self.srcs[0].view.float().clone()
            for b in self.srcs[1:W]:
                s += b.view.float()
            self.dense.view.copy_(s)
            K.adamw_apply(self.p.view, self.dense.view, self.m.view, self.v.view, LR, t, **kw)
        else:
            K.adamw_apply_multi(self.p.view, [b.view for b in self.srcs[:W]], self.m.view, self.v.view, LR, t, **kw)
        out = [b.view.clone() for b in (self.p, self.m, self.v)]
        if img_on:
            assert torch.equal(self.img.view, out[0].bfloat16()), "image"
        return out

    def check_untouched(self):
        assert all(b.intact() for b in (self.p, self.m, self.v, self.img, self.dense, *self.srcs)), "guard bands"
        assert all(torch.equal(b.view.cpu(), g.to(self.dtype)) for b, g in zip(self.srcs, self.cpu[3])), "sources"


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _check_config(rigs, n, dtype, W, t, wd):
    """One (W, t, wd) on every phase: bounds against the reference, and every form, with and
    without the image, from the W sources or the one dense source, in the same bits."""
    p, m, v, gs = _inputs(n)
    sc = K.adamw_scalars(LR, t, beta1=B1, beta2=B2, eps=EPS, wd=wd)
    s = _sum_fp32([g.to(dtype) for g in gs[:W]])
    ref = adamw_reference(p, m, v, s, sc, torch.tensor(1.0 / W, dtype=torch.float32).item())
    first = None
    for phase, rig in rigs.items():
        for img_on, dense in ((False, False), (True, False), (True, True)):
            out = rig.run(W, t, wd, img_on, dense)
            if first is None:
                first = out
                _note(assert_adamw_close(out[0], out[1], out[2], p, ref, sc, (n, dtype, W, t, wd)))
            else:
                assert _same(first, out), (n, dtype, W, t, wd, phase, img_on, dense)
    return first


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_update_matches_reference(n, dtype):
    rigs = {ph: Rig(n, dtype, ph) for ph in PHASES}
    for W in (1, 3, 7):
        for t in (1, 2, 1000):
            for wd in (0.0, 1e-2):
                _check_config(rigs, n, dtype, W, t, wd)
    a = rigs["aligned"].run(3, 2, 1e-2, True)
    assert _same(a, rigs["aligned"].run(3, 2, 1e-2, True))  # two runs on identical inputs
    for rig in rigs.values():
        rig.check_untouched()


@pytest.mark.parametrize("dtype,W", [(torch.float16, 3), (torch.float32, 1)])
def test_second_trip_of_the_capped_grid(dtype, W):
    """N_BIG elements: the grid-stride loop goes round again. The trip count does not interact
    with W, t or wd (scalars of the launch), so one configuration per source type, on all three
    phases; the other parameters are covered at the small sizes."""
    rigs = {ph: Rig(N_BIG, dtype, ph, nsrc=W) for ph in PHASES}
    _check_config(rigs, N_BIG, dtype, W, 2, 1e-2)
    for rig in rigs.values():
        rig.check_untouched()


def test_special_blocks():
    """s = m = v = 0: the element moves by the decay only, exactly p * decay (p itself with wd =
    0); p = 0: the plain Adam step from zero."""
    n = 2048
    p, m, v, gs = _inputs(n)
    rig = Rig(n, torch.float16, "shared")
    for wd in (0.0, 1e-2):
        decay = K.adamw_scalars(LR, 2, beta1=B1, beta2=B2, eps=EPS, wd=wd)[7]
        out = rig.run(3, 2, wd, True)
        want = p[:513] * torch.tensor(decay, dtype=torch.float32)
        assert decay == 1.0 if wd == 0.0 else decay < 1.0
        assert torch.equal(out[0][:513].cpu(), want)
        assert not bool(out[1][:513].any()) and not bool(out[2][:513].any())
        z = out[0][600:729].cpu()
        assert bool(torch.isfinite(z).all()) and bool((z != 0).all())


def test_capturable():
    """One launch on the caller's stream, no host synchronisation: captured into a HIP graph and
    replayed (one update, a fixed t), the bits equal the eager call."""
    n = 3 * 2048 + 5
    p0, m0, v0, gs = _inputs(n)
    srcs = [g.half().to(DEV) for g in gs[:3]]
    kw = dict(gscale=1 / 3, beta1=B1, beta2=B2, eps=EPS, wd=1e-2)
    res = []
    for graph in (False, True):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        img = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                K.adamw_apply_multi(p, srcs, m, v, LR, 5, img=img, **kw)
            for x, x0 in ((p, p0), (m, m0), (v, v0)):
                x.copy_(x0)
            g.replay()
        else:
            K.adamw_apply_multi(p, srcs, m, v, LR, 5, img=img, **kw)
        torch.cuda.synchronize()
        res.append([p.clone(), m.clone(), v.clone(), img.clone().view(torch.int16)])
    assert _same(res[0][:3], res[1][:3]) and torch.equal(res[0][3], res[1][3])


def test_argument_checks():
    n = 255
    p, m, v = (torch.ones(n, device=DEV) for _ in range(3))
    g = torch.ones(n, device=DEV)
    with pytest.raises(AssertionError):
        K.adamw_apply_multi(p, [g] * 33, m, v, LR, 1)
    with pytest.raises(AssertionError):
        K.adamw_apply_multi(p, [g, m], m, v, LR, 1)  # a source aliasing m
    with pytest.raises(AssertionError):
        K.adamw_apply_multi(p, [g, g.half()], m, v, LR, 1)
    with pytest.raises(AssertionError):
        K.adamw_apply_multi(p, [g], m, v, LR, 0)
    with pytest.raises(AssertionError):
        K.adamw_apply_multi(p[:-1], [g], m, v, LR, 1, n=n)
    # the C entry itself refuses, and launches nothing
    entry = K.kernels().psx_adamw_apply_multi
    st = torch.cuda.current_stream().cuda_stream

    def call(srcs, nsrc, mm, nn, t, pp=p):
        arr = (C.c_void_p * max(1, len(srcs)))(*[s.data_ptr() for s in srcs])
        return entry(pp.data_ptr() if pp is not None else None, arr, nsrc, 0, mm.data_ptr(), v.data_ptr(), nn, LR,
                     1.0, B1, B2, EPS, 0.0, t, None, st)

    assert call([g], 1, m, n, 0) != 0
    assert call([g], 1, m, 0, 1) != 0
    assert call([g], 0, m, n, 1) != 0
    assert call([g] * 33, 33, m, n, 1) != 0
    assert call([m], 1, m, n, 1) != 0
    assert call([p[8:]], 1, m, n, 1) != 0  # overlaps p without starting on it
    assert call([g], 1, m, n, 1, pp=None) != 0
    torch.cuda.synchronize()
    assert all(bool((x == 1).all()) for x in (p, m, v, g))
    assert call([g], 1, m, n, 1) == 0
    torch.cuda.synchronize()
    assert not bool((p == 1).any())


# ---------------------------------------------------------------------------- ParameterServer on the device
@pytest.mark.parametrize("kind", ["fp16", "q8", "topk"])
def test_server_paths_match_reference(kind):
    """The fp16 wire and a q8 / top-k payload (decoded into the aggregation buffer, one fp32
    source) against the fp64 reference on the decoded gradient, two pushes each."""
    s, lay, cfg = _tiny_server(device=DEV, codec=kind, topk_ratio=0.25)
    n = lay.param_numel
    for step, (wire, dense) in enumerate(wires(kind, n, 2, cfg, device=DEV)):
        sc = server_scalars(cfg, step + 1)
        p_old = s.params.cpu()
        ref = adamw_reference(p_old, s.adam_m.cpu(), s.adam_v.cpu(), dense.cpu(), sc, 0.5)
        s.apply(wire, 0.5)
        _note(assert_adamw_close(s.params, s.adam_m, s.adam_v, p_old, ref, sc, (kind, step)))
    assert s.adam_t == 2 and s.final_metrics()["adamw"]["steps"] == 2


def test_server_ranges_equal_the_whole_round():
    a_srv, lay, cfg = _tiny_server(device=DEV, codec="fp16")
    b_srv, _, _ = _tiny_server(device=DEV, codec="fp16")
    n = lay.param_numel
    a, b = n // 3 | 1, (2 * n // 3) | 1
    gen = torch.Generator().manual_seed(5)
    for rnd in range(2):
        srcs = [(torch.randn(n, generator=gen) * 1e-2).half().to(DEV) for _ in range(2)]
        a_srv.apply_range_sources(srcs, 0.5, 0, n)
        a_srv.finish_round_apply()
        for lo, hi in ((0, a), (a, b), (b, n)):
            b_srv.apply_range_sources(srcs, 0.5, lo, hi)
        b_srv.finish_round_apply()
        assert a_srv.adam_t == b_srv.adam_t == rnd + 1
        assert torch.equal(a_srv.arena, b_srv.arena)
        assert torch.equal(a_srv.adam_m, b_srv.adam_m) and torch.equal(a_srv.adam_v, b_srv.adam_v)


def test_server_weight_image():
    """With the weight-image fetch path on, the apply writes the bf16 image in the same pass, also
    when the round arrives as ranges."""
    s, lay, cfg = _tiny_server(device=DEV, codec="fp16", dtype="bf16")
    n = lay.param_numel
    s.enable_weight_wire()
    before = s.params.clone()
    g = (torch.randn(n, generator=torch.Generator().manual_seed(3)) * 1e-2).half().to(DEV)
    s.apply(g, 1.0)
    assert not s._wire_stale and not torch.equal(before, s.params)
    assert torch.equal(s.wire.img[:n], s.params.bfloat16())
    for lo, hi in ((0, n // 2 | 1), (n // 2 | 1, n)):
        s.apply_range_sources([g, g], 0.5, lo, hi)
    s.finish_round_apply()
    assert not s._wire_stale and torch.equal(s.wire.img[:n], s.params.bfloat16())


def test_server_checkpoint_resume(tmp_path):
    kw = dict(device=DEV, codec="none", ckpt_dir=str(tmp_path))
    a, lay, _ = _tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2 = ((torch.randn(lay.param_numel, generator=gen) * 1e-2).to(DEV) for _ in range(2))
    a.apply(g1, 1.0)
    path = a.checkpoint()
    a.apply(g2, 1.0)
    b, _, _ = _tiny_server(**kw)
    b.resume(path)
    assert b.adam_t == 1
    b.apply(g2, 1.0)
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert a.adam_t == b.adam_t == 2
