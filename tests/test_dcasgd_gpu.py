"""Delay-compensated async updates (--dc-lambda, csrc/kernels/dcasgd.hip) on the MI355X:

* dc_apply against an fp64 evaluation of the formula, element by element within
  16 * 2^-24 * M (M: the sum of the magnitudes the update adds up), for every instantiation
  (fp16 / fp32 wire x momentum off / first step / running x constant / adaptive x bf16 image on /
  off), the ragged sizes, and a size at which the grid-stride loop runs more than twice;
* staleness 0, dc_fetch_copy, graph capture, argument checks;
* a scripted three-worker schedule through the native event loop, the Python loop and direct
  calls: the same decisions, counts and bits, and a CPU-arena server to a tolerance;
* worker threads on the native loop (run_local_threads) with compensation on;
* two remote workers on the native loop at world 3 (the fetch snapshot that leaves the backup).
"""
import queue
import threading
import uuid

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from psx.ops import kernels as K  # noqa: E402

U = 2.0 ** -24
N_LARGE = 11_220_132  # ResNet-18 (100 classes): n/8 lanes > 2 x (2048 workgroups x 256 lanes), n % 8 = 4
SIZES = [1, 7, 8, 9, 1027, N_LARGE]
LR, GSCALE, WD, MOM, DECAY, EPS = 0.05, 0.7, 5e-4, 0.9, 0.95, 1e-7


def f32(x) -> float:
    """A hyper-parameter as the kernels' C ABI receives it (a float)."""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def data():
    """The inputs of every kernel test, generated once (sizes below N_LARGE are prefixes):
    g ~ N(0,1), p ~ N(0,1), bak = p + 0.1 N(0,1), buf ~ N(0,1), ms ~ U(0.5, 2). Never written."""
    gen = torch.Generator(device="cuda").manual_seed(1234)
    r = lambda: torch.randn(N_LARGE, generator=gen, device="cuda")  # noqa: E731
    g, p = r(), r()
    d = dict(g32=g, g16=g.half(), p=p, bak=p + 0.1 * r(), buf=r(),
             ms=0.5 + 1.5 * torch.rand(N_LARGE, generator=gen, device="cuda"))
    torch.cuda.synchronize()
    return d


def ref64(g, p, bak, ms, buf, lam, first):
    """The update in fp64 on the device, from the definition, with the scalars the kernel gets
    (fp32 values). Returns p', ms', buf', and the bounds' magnitudes M_p, M_ms, M_buf."""
    lr, gs, wd, mom, decay, eps, lam = (f32(x) for x in (LR, GSCALE, WD, MOM, DECAY, EPS, lam))
    g, p, bak = g.double(), p.double(), bak.double()
    lam_e, ms_new, m_ms = lam, None, None
    if ms is not None:
        ms_new = decay * ms.double() + (1.0 - decay) * g * g
        m_ms = ms_new
        lam_e = lam / torch.sqrt(ms_new + eps)
    gt = g + lam_e * g * g * (p - bak)
    d = gs * gt + wd * p
    m_d = gs * (g.abs() + lam_e * g * g * (p - bak).abs()) + wd * p.abs()
    buf_new = None
    if buf is not None:
        if not first:
            d = mom * buf.double() + d
            m_d = m_d + mom * buf.double().abs()
        buf_new = d
    return p - lr * d, ms_new, buf_new, p.abs() + lr * m_d, m_ms, m_d


def _within(out, ref, m, what):
    err = (out.double() - ref).abs()
    bad = err > 16 * U * m
    worst = float((err / (U * m)).max())
    print(f"{what}: max |err| / (2^-24 M) = {worst:.2f}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


@pytest.mark.parametrize("img_on", [True, False])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("mom_mode", ["none", "first", "running"])
@pytest.mark.parametrize("wire", ["fp16", "fp32"])
def test_dc_apply_matches_fp64(data, wire, mom_mode, adaptive, img_on):
    for n in SIZES:
        for lam in (0.5, 2.0):
            g = data["g16" if wire == "fp16" else "g32"][:n]
            p, bak = data["p"][:n].clone(), data["bak"][:n]
            ms = data["ms"][:n].clone() if adaptive else None
            buf = data["buf"][:n].clone() if mom_mode != "none" else None
            first = mom_mode == "first"
            img = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if img_on else None
            rp, rms, rbuf, m_p, m_ms, m_buf = ref64(g, data["p"][:n], bak, ms, buf, lam, first)
            r0 = ref64(g, data["p"][:n], bak, ms, buf, 0.0, first)[0]  # the same update without compensation
            K.dc_apply(p, g, bak, LR, lam, ms=ms, decay=DECAY, eps=EPS, gscale=GSCALE,
                       momentum=MOM if buf is not None else 0.0, wd=WD, buf=buf, first=first, n=n, img=img)
            tag = f"{wire} {mom_mode} adaptive={adaptive} img={img_on} n={n} lam={lam}"
            _within(p, rp, m_p, "p " + tag)
            if adaptive:
                _within(ms, rms, m_ms, "ms " + tag)
            if buf is not None:
                _within(buf, rbuf, m_buf, "buf " + tag)
            if img_on:  # bitwise the round-to-nearest-even bf16 of the kernel's own fp32 output
                assert torch.equal(img.view(torch.int16), p.to(torch.bfloat16).view(torch.int16)), tag
            if n >= 1027:  # compensation was applied: far from the lambda = 0 result for most elements
                moved = ((rp - r0).abs() > 100 * 16 * U * m_p).double().mean().item()
                far = ((p.double() - r0).abs() > 100 * 16 * U * m_p).double().mean().item()
                print(f"compensated elements {tag}: {far:.3f} (reference {moved:.3f})")
                assert far > 0.5, (tag, far)


def test_dc_apply_unaligned_and_no_backup(data):
    """Base pointers off the 16-byte grid take the scalar form; bak None leaves g uncompensated
    while the adaptive form still updates ms. Same bound."""
    n = 1027
    g = data["g16"][1:n + 1]
    p, bak = data["p"][1:n + 1].clone(), data["bak"][1:n + 1]
    ms, buf = data["ms"][1:n + 1].clone(), data["buf"][1:n + 1].clone()
    hold = [torch.empty(n + 1, device="cuda") for _ in range(3)]  # views starting 4 bytes into an allocation
    for h, t in zip(hold, (p, ms, buf)):
        h[1:].copy_(t)
    p, ms, buf = (h[1:] for h in hold)
    assert p.data_ptr() % 16 == 4
    rp, rms, rbuf, m_p, m_ms, m_buf = ref64(g, data["p"][1:n + 1], bak, data["ms"][1:n + 1], data["buf"][1:n + 1],
                                            2.0, False)
    K.dc_apply(p, g, bak, LR, 2.0, ms=ms, decay=DECAY, eps=EPS, gscale=GSCALE, momentum=MOM, wd=WD, buf=buf, n=n)
    _within(p, rp, m_p, "p unaligned")
    _within(ms, rms, m_ms, "ms unaligned")
    _within(buf, rbuf, m_buf, "buf unaligned")
    # no backup: the reference with bak = p (zero compensation), ms still moves
    p2, ms2 = data["p"][:n].clone(), data["ms"][:n].clone()
    rp, rms, _, m_p, m_ms, _ = ref64(data["g32"][:n], p2, p2, ms2, None, 2.0, False)
    K.dc_apply(p2, data["g32"][:n], None, LR, 2.0, ms=ms2, decay=DECAY, eps=EPS, gscale=GSCALE, wd=WD, n=n)
    _within(p2, rp, m_p, "p no backup")
    _within(ms2, rms, m_ms, "ms no backup")
    assert not torch.equal(ms2, data["ms"][:n])


@pytest.mark.parametrize("wire", ["fp16", "fp32"])
@pytest.mark.parametrize("n", [9, 1027, N_LARGE])
def test_staleness_zero(data, wire, n):
    """bak bitwise equal to p: the constant form gives the bits of lambda = 0, and both agree
    with sgd_apply within the bound."""
    g = data["g16" if wire == "fp16" else "g32"][:n]
    p0 = data["p"][:n]
    a, b, c = p0.clone(), p0.clone(), p0.clone()
    K.dc_apply(a, g, p0, LR, 2.0, gscale=GSCALE, wd=WD, n=n)
    K.dc_apply(b, g, p0, LR, 0.0, gscale=GSCALE, wd=WD, n=n)
    K.sgd_apply(c, g, LR, gscale=GSCALE, wd=WD, n=n)
    assert torch.equal(a, b)
    rp, _, _, m_p, _, _ = ref64(g, p0, p0, None, None, 0.0, False)
    _within(a, rp, m_p, f"dc staleness 0 {wire} n={n}")
    _within(c, rp, m_p, f"sgd {wire} n={n}")


@pytest.mark.parametrize("with_dst", [True, False])
@pytest.mark.parametrize("n_params,n_arena", [(1, 1), (7, 7), (5, 7), (1027, 1027), (1027, 1093), (1026, 1093),
                                              (N_LARGE, N_LARGE), (N_LARGE - 9601, N_LARGE)])
def test_dc_fetch_copy(data, n_params, n_arena, with_dst):
    src = data["p"][:n_arena]
    guard = 3
    bak = torch.full((n_params + guard,), -7.0, device="cuda")
    dst = torch.full((n_arena + guard,), -7.0, device="cuda") if with_dst else None
    K.dc_fetch_copy(src, dst[:n_arena] if with_dst else None, bak[:n_params], n_params)
    assert torch.equal(bak[:n_params].view(torch.int32), src[:n_params].view(torch.int32))
    assert bool((bak[n_params:] == -7.0).all())  # nothing beyond n_params of the backup is written
    if with_dst:
        assert torch.equal(dst[:n_arena].view(torch.int32), src.view(torch.int32))
        assert bool((dst[n_arena:] == -7.0).all())


def test_dc_fetch_copy_writes_no_more_than_n_params_of_a_larger_backup(data):
    src = data["p"][:1093]
    bak = torch.full((1093,), -7.0, device="cuda")
    K.dc_fetch_copy(src, None, bak, 1027)
    assert torch.equal(bak[:1027], src[:1027]) and bool((bak[1027:] == -7.0).all())


def test_dc_apply_graph_capture(data):
    """Recorded in a HIP graph and replayed twice = two eager calls, bit for bit."""
    n = 1027 * 33 + 5
    g, bak = data["g16"][:n], data["bak"][:n]

    def state():
        return (data["p"][:n].clone(), data["ms"][:n].clone(), data["buf"][:n].clone(),
                torch.zeros(n, dtype=torch.bfloat16, device="cuda"))

    def call(p, ms, buf, img):
        K.dc_apply(p, g, bak, LR, 2.0, ms=ms, decay=DECAY, eps=EPS, gscale=GSCALE, momentum=MOM, wd=WD, buf=buf,
                   first=False, n=n, img=img)

    eager = state()
    call(*eager)
    call(*eager)
    cap = state()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call(*cap)
    for t, src in zip(cap, state()):  # a capture does not run: restore the inputs anyway
        t.copy_(src)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


def test_argument_checks(data):
    n = 1027
    p, g, bak = data["p"][:n].clone(), data["g16"][:n], data["bak"][:n]
    ok = dict(lr=LR, lam=0.5)
    with pytest.raises(AssertionError):  # wrong dtypes
        K.dc_apply(p.double(), g, bak, **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g.to(torch.bfloat16), bak, **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak.half(), **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak, ms=data["ms"][:n].double(), **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak, img=torch.zeros(n, dtype=torch.float16, device="cuda"), **ok)
    with pytest.raises(AssertionError):  # short buffers
        K.dc_apply(p, g[: n - 1], bak, **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak[: n - 1], **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak, buf=data["buf"][: n - 1], momentum=0.9, **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p, g, bak, img=torch.zeros(n - 1, dtype=torch.bfloat16, device="cuda"), **ok)
    with pytest.raises(AssertionError):  # device mismatch
        K.dc_apply(p, g, bak.cpu(), **ok)
    with pytest.raises(AssertionError):
        K.dc_apply(p.cpu(), g.cpu(), bak.cpu(), **ok)
    with pytest.raises(AssertionError):  # not contiguous
        K.dc_apply(p, g, data["bak"][: 2 * n: 2], **ok)
    with pytest.raises(AssertionError):
        K.dc_fetch_copy(p, None, bak[: n - 1])
    with pytest.raises(AssertionError):
        K.dc_fetch_copy(p, torch.empty(n - 1, device="cuda"), torch.empty(n, device="cuda"))
    with pytest.raises(AssertionError):
        K.dc_fetch_copy(p, None, torch.empty(n))
    with pytest.raises(AssertionError):
        K.dc_fetch_copy(p, None, torch.empty(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        K.dc_fetch_copy(p, None, torch.empty(n + 1, device="cuda"), n_params=n + 1)  # past the arena
    assert torch.equal(p, data["p"][:n])  # no refused call touched the parameters


# ---------------------------------------------------------------------------- server paths
W = 3
# (kind, worker, local step), staleness bound 2. Starts with fetches; worker 2 never fetches (its
# pushes have no backup: uncompensated). Pushes: fresh (staleness 0), stale but accepted (1-2),
# rejected (above the bound).
SCHEDULE = [("f", 0, 0), ("f", 1, 0), ("p", 0, 0), ("p", 1, 0), ("p", 2, 1), ("f", 0, 0), ("p", 0, 3), ("p", 1, 0),
            ("f", 1, 0), ("p", 2, 3), ("p", 1, 4), ("p", 0, 3), ("f", 0, 0), ("p", 0, 6), ("p", 1, 5), ("p", 2, 0)]


def _server(device, momentum, lam, adaptive):
    from psx.parallel.runner import build_state
    from psx.parallel.server import ParameterServer
    from psx.utils.config import PSConfig

    cfg = PSConfig(model="resnet_tiny", mode="async", workers=W, lr=0.05, staleness_bound=2, codec="fp16",
                   momentum=momentum, weight_decay=5e-4 if momentum else 0.0, eval_every=0, verbose=0,
                   heartbeat_timeout=0, dc_lambda=lam, dc_adaptive=adaptive).validate()
    _, lay, arena, counters = build_state(cfg)
    srv = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=W, log=lambda *a, **k: None)
    for w in range(W):
        srv.register_worker(f"w{w}", w)
    gen = torch.Generator().manual_seed(7)
    grads = [(torch.randn(srv.n, generator=gen) * 0.5).half().to(device) for _ in SCHEDULE]
    return srv, lay, grads


def _drive(how: str, momentum: float, lam: float, adaptive: bool):
    """The schedule through 'native' (NativeServerLoop + NativeLocalChannel), 'python'
    (serve_async + LocalAsyncChannel), 'direct' (push_gradients / fetch_parameters) or 'cpu'
    (direct, CPU arena)."""
    from psx.parallel import control as CP
    from psx.parallel.native_loop import NativeLocalChannel, NativeServerLoop
    from psx.parallel.worker import LocalAsyncChannel

    device = "cpu" if how == "cpu" else "cuda"
    srv, lay, grads = _server(device, momentum, lam, adaptive)
    local = torch.empty(lay.arena_numel, device=device)
    trace, fetched = [], []  # fetched: the sum of what each fetch delivered (equal bits -> equal sums)
    path = srv.arena.abs().double()  # |p0| + sum over the applies of |p_k+1 - p_k| (direct / cpu only)
    if how in ("direct", "cpu"):
        for i, (kind, w, ls) in enumerate(SCHEDULE):
            if kind == "p":
                before = srv.arena.clone()
                trace.append(("p", bool(srv.push_gradients(w, grads[i], ls)), srv.core.global_step))
                path += (srv.arena.double() - before.double()).abs()
            else:
                arena, gs = srv.fetch_parameters(w)
                local.copy_(arena)
                trace.append(("f", gs))
                fetched.append(float(local.double().sum()))
    else:
        mbox = CP.ShmMailbox(f"/psx_t{uuid.uuid4().hex[:10]}", nreply=1, owner=True)
        try:
            if how == "native":
                loop = NativeServerLoop(srv, None, mbox, {}, W, update_stream=torch.cuda.current_stream())
                ch = NativeLocalChannel(srv, loop)
            else:
                q = queue.Queue()
                th = threading.Thread(target=srv.serve_async, args=(None, mbox, {}),
                                      kwargs={"local_queue": q, "expected": W}, daemon=True)
                th.start()
                ch = LocalAsyncChannel(srv, q)
            for i, (kind, w, ls) in enumerate(SCHEDULE):
                if kind == "p":
                    trace.append(("p", bool(ch.push(w, grads[i], ls)), srv.core.global_step))
                else:
                    trace.append(("f", ch.fetch(w, local)))
                    fetched.append(float(local.double().sum()))
            for w in range(W):
                ch.finished(w)
            if how == "native":
                loop.join()
            else:
                th.join(timeout=60)
        finally:
            mbox.close()
    if device == "cuda":
        torch.cuda.synchronize()
    m = srv.final_metrics()
    return dict(trace=trace, fetched=fetched, hist=srv.core.staleness_histogram(), steps=srv.core.global_step,
                dc=m.get("delay_compensation"), sha=m["final_param_sha256"], arena=srv.arena.cpu().clone(),
                path=path.cpu(),
                ms=None if srv._dc_ms is None else srv._dc_ms.cpu().clone())


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_scripted_schedule_three_ways(momentum, adaptive):
    lam = 2.0 if adaptive else 0.5
    nat, py, direct = (_drive(how, momentum, lam, adaptive) for how in ("native", "python", "direct"))
    pushes = [t for t in direct["trace"] if t[0] == "p"]
    accepted = sum(1 for t in pushes if t[1])
    assert 0 < accepted < len(pushes)  # the schedule rejects some pushes
    hist = direct["hist"]
    assert hist[0] > 0 and sum(hist[1:]) > 0  # fresh and stale accepted pushes
    for other in (nat, py):
        assert other["trace"] == direct["trace"], (other["trace"], direct["trace"])
        assert other["fetched"] == direct["fetched"]  # the fetch that leaves the backup delivers the arena
        assert other["hist"] == hist and other["steps"] == direct["steps"] == accepted
        assert other["dc"] == direct["dc"], (other["dc"], direct["dc"])
        assert torch.equal(other["arena"], direct["arena"]) and other["sha"] == direct["sha"]
        if adaptive:
            assert torch.equal(other["ms"], direct["ms"])
    dc = direct["dc"]
    assert dc["lambda"] == lam and dc["adaptive"] is adaptive
    assert dc["uncompensated_pushes"] >= 1 and dc["compensated_pushes"] >= 4
    assert dc["compensated_pushes"] + dc["uncompensated_pushes"] == accepted
    # a CPU-arena server on the same schedule (the torch formula): equal to a tolerance
    cpu = _drive("cpu", momentum, lam, adaptive)
    assert cpu["trace"] == direct["trace"] and cpu["dc"] == dc
    # rtol 1e-5, relative to what each element's value was summed from: its start and the steps it
    # took (|p0| + sum |p_k+1 - p_k|). Relative to the end value alone no two fp32 evaluations of a
    # sum agree: elements that land near zero differ by 1e-3 of themselves at 1.5e-8 absolute.
    diff = (cpu["arena"].double() - direct["arena"].double()).abs()
    print(f"cpu vs device arena, momentum={momentum} adaptive={adaptive}: max |diff| {diff.max().item():.3e}, "
          f"max |diff| / path {(diff / direct['path'].clamp_min(1e-300)).max().item():.3e}, max |diff| / |value| "
          f"{(diff / direct['arena'].double().abs().clamp_min(1e-300)).max().item():.3e}")
    assert bool((diff <= 1e-5 * direct["path"]).all())
    # without compensation the same schedule ends somewhere else
    plain = _drive("direct", momentum, 0.0, False)
    assert plain["trace"] == direct["trace"] and plain["dc"] is None
    assert plain["sha"] != direct["sha"]


# ---------------------------------------------------------------------------- worker threads
def test_threads_async_with_dc():
    from psx.parallel.runner import run_local_threads
    from psx.utils.config import PSConfig

    Wt, steps = 3, 4
    cfg = PSConfig(model="resnet18", mode="async", workers=Wt, lr=0.05, batch_size=32, epochs=1, train_samples=2048,
                   eval_every=0, verbose=0, staleness_bound=5, dc_lambda=0.04).validate()
    s = run_local_threads(cfg, steps, log=lambda *a, **k: None, emit=False)["server"]
    assert np.isfinite(s["final_param_checksum"])
    dc = s["delay_compensation"]
    assert dc["lambda"] == 0.04 and dc["adaptive"] is False
    assert dc["compensated_pushes"] + dc["uncompensated_pushes"] == s["async_updates"] > 0, s
    assert dc["compensated_pushes"] > 0  # every thread worker fetches before it pushes
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- remote workers
_REMOTE = r"""
import json, sys
sys.path.insert(0, {root!r})
import psx
from psx.parallel.runner import run_distributed
from psx.utils.config import PSConfig
cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=0, lr=0.05,
               max_steps=4, mode="async", topology="dedicated", heartbeat_timeout=0, use_graph=True, dtype={dtype!r},
               dc_lambda=2.0, dc_adaptive={adaptive}).validate()
res = run_distributed(cfg, log=lambda *a, **k: None)
if "server" in res:
    s, dc = res["server"], res["server"]["delay_compensation"]
    print("RESULT " + json.dumps([s["async_updates"], s["rejected_pushes"], s["gradients_processed"],
                                 s["final_param_checksum"], dc["compensated_pushes"], dc["uncompensated_pushes"]]))
"""


@pytest.mark.parametrize("dtype,adaptive", [("fp32", False), ("bf16", True)])
def test_remote_workers_native_loop_with_dc(dtype, adaptive, tmp_path):
    """World 3, dedicated server, two remote workers on the native event loop (the multi-process
    stand-in communicator of tests/test_multirank_gpu.py): serve_fetch leaves the backup from the
    fp32 snapshot copy (fp32 fetch) or by a backup-only pass (bf16conv fetch), and every accepted
    push is compensated (a worker fetches before it pushes)."""
    from .test_multirank_gpu import ROOT, _json_lines, _torchrun

    script = tmp_path / "dc_remote.py"
    script.write_text(_REMOTE.format(root=ROOT, dtype=dtype, adaptive=adaptive))
    out = _torchrun(3, [str(script)], extra={"PSX_NATIVE_LOOP": "1", "PSX_FAKECOMM_TIMEOUT_S": "240"})
    recs = [r for r in _json_lines(out, "RESULT ") if r]
    assert len(recs) == 1, out[-3000:]
    applied, rejected, processed, checksum, comp, uncomp = recs[0]
    assert processed == 2 * 4 and applied + rejected == processed and applied > 0, recs
    assert comp == applied and uncomp == 0, recs
    assert np.isfinite(checksum) and abs(checksum) < 1e12
