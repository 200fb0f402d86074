"""Delay-compensated async updates (--dc-lambda, DC-ASGD) on the CPU path: configuration scope,
the torch implementation in ParameterServer against a numpy fp64 implementation of the formula
written here, checkpoint / resume of the mean square, the metrics record, and the loopback run.
The fp64 reference (dc_reference) is shared with the GPU kernel tests."""
import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel.server import ParameterServer
from psx.utils import checkpoint as ckpt
from psx.utils.config import PSConfig, parse

from .test_ps_cpu import tiny_cfg


def dc_reference(p, g, bak, ms, buf, *, lr, gscale, momentum, wd, lam, decay, eps, first):
    """One delay-compensated update in fp64 (numpy), straight from the definition. p, g: arrays;
    bak: the worker's backup or None (uncompensated); ms: the mean square or None (constant
    form); buf: the momentum buffer or None. Returns (p_new, ms_new, buf_new, g_tilde)."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    ms_new = None
    lam_e = lam
    if ms is not None:
        ms_new = decay * np.asarray(ms, np.float64) + (1.0 - decay) * g * g
        lam_e = lam / np.sqrt(ms_new + eps)
    gt = g + lam_e * g * g * (p - np.asarray(bak, np.float64)) if bak is not None else g
    d = gscale * gt + wd * p
    buf_new = None
    if momentum and buf is not None:
        d = d if first else momentum * np.asarray(buf, np.float64) + d
        buf_new = d
    return p - lr * d, ms_new, buf_new, gt


# ---------------------------------------------------------------------------- configuration
def test_validate_scope():
    ok = PSConfig(mode="async", dc_lambda=0.04).validate()
    assert (ok.dc_lambda, ok.dc_adaptive, ok.dc_decay, ok.dc_eps) == (0.04, False, 0.95, 1e-7)
    assert PSConfig(mode="async", dc_lambda=2.0, dc_adaptive=True, dc_decay=0.0).validate().dc_adaptive
    assert PSConfig(mode="sync").validate().dc_lambda == 0.0  # off by default, in either mode
    assert PSConfig(mode="async").validate().dc_lambda == 0.0
    assert PSConfig(mode="async", dc_lambda=0.04, momentum=0.9, codec="q8").validate().codec == "q8"
    for bad in (dict(mode="async", dc_lambda=-0.1),
                dict(mode="sync", dc_lambda=0.04),
                dict(mode="async", dc_lambda=0.04, optimizer="lars"),
                dict(mode="async", dc_adaptive=True),
                dict(mode="async", dc_lambda=0.04, dc_decay=1.0),
                dict(mode="async", dc_lambda=0.04, dc_decay=-0.01),
                dict(mode="async", dc_decay=1.5)):
        with pytest.raises(ValueError):
            PSConfig(**bad).validate()


def test_cli_flags():
    cfg = parse(["--mode", "async", "--dc-lambda", "2", "--dc-adaptive", "--dc-decay", "0.9", "--dc-eps", "1e-6"])
    assert (cfg.dc_lambda, cfg.dc_adaptive, cfg.dc_decay, cfg.dc_eps) == (2.0, True, 0.9, 1e-6)
    assert parse(["--mode", "async"]).dc_lambda == 0.0
    with pytest.raises(ValueError):
        parse(["--dc-lambda", "0.04"])  # the default mode is sync


def test_native_loop_keeps_serving_dc_jobs():
    import types

    from psx.parallel.native_loop import native_loop_enabled

    t = types.SimpleNamespace(native=True)
    assert native_loop_enabled(PSConfig(mode="async", dc_lambda=0.04).validate(), t)
    assert native_loop_enabled(PSConfig(mode="async", dc_lambda=2.0, dc_adaptive=True, momentum=0.9).validate(), t)


# ---------------------------------------------------------------------------- server numerics
W = 3
# (kind, worker, local step): worker 2 pushes before its first fetch (no backup: uncompensated);
# later pushes carry staleness 0 (fresh), 1-3 (stale, accepted) and one above the bound (rejected)
SCHEDULE = [("f", 0, 0), ("f", 1, 0), ("p", 2, 0), ("p", 0, 0), ("p", 1, 0), ("f", 0, 0), ("p", 0, 3), ("f", 2, 0),
            ("p", 1, 1), ("p", 2, 4), ("f", 1, 0), ("p", 1, 0), ("p", 0, 4), ("f", 0, 0), ("p", 0, 7), ("p", 2, 6)]


def _tiny_server(**kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(mode="async", workers=W, staleness_bound=3, codec="none", **kw)
    s = ParameterServer(cfg, lay, arena.clone(), counters, total_workers=W, log=lambda *a: None)
    for w in range(W):
        s.register_worker(f"w{w}", w)
    return s, lay, cfg


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_torch_path_matches_numpy_fp64(adaptive, momentum):
    """push_gradients / fetch_parameters on a CPU arena over SCHEDULE against the fp64 formula.
    Tolerance: every fp32 step rounds a handful of times at 2^-24 relative to the parameter, and
    the schedule has 9 applies: rtol 1e-5 (+ 1e-7 absolute for parameters that start at zero)."""
    lam = 2.0
    kw = dict(dc_lambda=lam, dc_adaptive=adaptive, momentum=momentum, weight_decay=5e-4 if momentum else 0.0, lr=0.05)
    s, lay, cfg = _tiny_server(**kw)
    n = lay.param_numel
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=gen) * 0.5 for _ in SCHEDULE]
    p = s.params.double().numpy().copy()
    p_plain = p.copy()  # the same schedule without compensation (lambda = 0)
    ms = np.zeros(n) if adaptive else None
    buf, buf_plain = (np.zeros(n), np.zeros(n)) if momentum else (None, None)
    bak, first = {}, True
    comp = uncomp = rejected = 0
    for (kind, w, ls), g in zip(SCHEDULE, grads):
        if kind == "f":
            arena, _ = s.fetch_parameters(w)
            assert arena is s.arena
            bak[w] = p.copy()
            continue
        ok = s.push_gradients(w, g, ls)
        if not ok:
            rejected += 1
            continue
        kwr = dict(lr=cfg.lr, gscale=s.last_push.weight, momentum=momentum, wd=cfg.weight_decay, decay=cfg.dc_decay,
                   eps=cfg.dc_eps, first=first)
        p_plain, _, buf_plain, _ = dc_reference(p_plain, g.numpy(), None, None, buf_plain, lam=0.0, **kwr)
        p, ms, buf, _ = dc_reference(p, g.numpy(), bak.get(w), ms, buf, lam=lam, **kwr)
        first = False
        comp += w in bak
        uncomp += w not in bak
        np.testing.assert_allclose(s.params.numpy(), p, rtol=1e-5, atol=1e-7)
    assert rejected >= 1 and uncomp == 1 and comp >= 6
    if adaptive:
        np.testing.assert_allclose(s._dc_ms.numpy(), ms, rtol=1e-5, atol=1e-12)
    if momentum:
        # momentum * buf + d cancels for some elements, so the error is relative to the summands
        # (|g| up to ~2.5, buffers up to ~3), not to the result: 9 applies x 3 roundings x 2^-24 x 3
        np.testing.assert_allclose(s.momentum_buf.numpy(), buf, rtol=1e-5, atol=5e-6)
    # the compensation is far above the tolerance: the lambda = 0 trajectory is somewhere else
    # (element by element, over 100x the tolerance for more than a quarter of the parameters)
    assert (np.abs(p - p_plain) > 100 * (1e-5 * np.abs(p) + 1e-7)).mean() > 0.25
    dc = s.final_metrics()["delay_compensation"]
    assert dc == {"lambda": lam, "adaptive": adaptive, "compensated_pushes": comp, "uncompensated_pushes": uncomp}
    assert comp + uncomp == s.core.metrics()["async_updates"]


def test_staleness_zero_is_plain_sgd():
    """A push right after the worker's own fetch: w == bak, so the update is the plain one."""
    a, lay, _ = _tiny_server(dc_lambda=2.0)
    b, _, _ = _tiny_server()
    g = torch.randn(lay.param_numel, generator=torch.Generator().manual_seed(1)) * 0.1
    for s in (a, b):
        s.fetch_parameters(0)
        assert s.push_gradients(0, g, 0)
    assert torch.equal(a.arena, b.arena)
    assert a.dc_compensated == 1 and "delay_compensation" not in b.final_metrics()


@pytest.mark.parametrize("codec", ["q8", "topk"])
def test_payloads_are_decoded_then_compensated(codec):
    """q8 / top-k payloads go through the aggregation buffer and the same formula (the top-k
    scatter-into-the-parameters shortcut is not taken)."""
    from psx.parallel import q8 as Q
    from psx.parallel import topk as T

    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(mode="async", workers=2, staleness_bound=5, codec=codec, topk_ratio=0.25, dc_lambda=2.0, lr=0.05)
    s = ParameterServer(cfg, lay, arena.clone(), counters, total_workers=2, log=lambda *a: None)
    n = lay.param_numel
    enc = Q.Q8Codec(n) if codec == "q8" else T.TopKCodec(n, cfg.topk_ratio, "cpu")
    gen = torch.Generator().manual_seed(3)
    for w in range(2):
        s.register_worker(f"w{w}", w)
        s.fetch_parameters(w)
    p = s.params.double().numpy().copy()
    bak = p.copy()
    for w in range(2):  # worker 1's push is stale by one update
        enc.resid.zero_()
        wire = enc.encode(torch.randn(n, generator=gen) * 0.1).clone()
        dense = (Q.decode(wire, n) if codec == "q8"
                 else T.decode_add(wire, torch.zeros(n), 1.0, T.topk_k(n, cfg.topk_ratio))).clone()
        assert s.push_gradients(w, wire, 0)
        p, _, _, _ = dc_reference(p, dense.numpy(), bak, None, None, lr=cfg.lr, gscale=s.last_push.weight,
                                  momentum=0.0, wd=0.0, lam=2.0, decay=0.95, eps=1e-7, first=False)
        np.testing.assert_allclose(s.params.numpy(), p, rtol=1e-5, atol=1e-7)
    assert s.dc_compensated == 2


# ---------------------------------------------------------------------------- checkpoint / resume
def test_checkpoint_carries_meansquare(tmp_path):
    kw = dict(dc_lambda=2.0, dc_adaptive=True, momentum=0.9, lr=0.05, ckpt_dir=str(tmp_path))
    a, lay, _ = _tiny_server(**kw)
    gen = torch.Generator().manual_seed(8)
    g1, g2 = (torch.randn(lay.param_numel, generator=gen) * 0.1 for _ in range(2))
    a.fetch_parameters(0)
    a.push_gradients(0, g1, 0)
    path = a.checkpoint()
    saved = ckpt.load(path)["server_optimizer_state"]
    assert torch.equal(saved["dc_meansquare"], a._dc_ms) and float(saved["dc_meansquare"].abs().sum()) > 0
    b, _, _ = _tiny_server(**kw)
    b.fetch_parameters(0)  # a backup from before the resume must not survive it
    b.resume(path)
    assert torch.equal(b._dc_ms, a._dc_ms) and torch.equal(b.arena, a.arena) and not b._dc_valid
    # the push after a resume has no backup: uncompensated on both (a: worker 1 never fetched)
    a.push_gradients(1, g2, 1)
    b.push_gradients(1, g2, 1)
    assert torch.equal(a.arena, b.arena) and torch.equal(a._dc_ms, b._dc_ms)
    assert b.dc_uncompensated == 1 and b.dc_compensated == 0


def test_checkpoint_without_the_key_loads(tmp_path):
    plain, lay, _ = _tiny_server(momentum=0.9, ckpt_dir=str(tmp_path))
    plain.push_gradients(0, torch.ones(lay.param_numel) * 0.01, 0)
    path = plain.checkpoint()
    assert "dc_meansquare" not in ckpt.load(path)["server_optimizer_state"]
    s, _, _ = _tiny_server(dc_lambda=2.0, dc_adaptive=True, momentum=0.9, ckpt_dir=str(tmp_path))
    s.resume(path)
    assert torch.equal(s.arena, plain.arena) and float(s._dc_ms.abs().sum()) == 0.0
    assert s.core.global_step == 1


# ---------------------------------------------------------------------------- loopback runs
def _loopback(**kw):
    from psx.parallel.runner import run_local

    cfg = tiny_cfg(mode="async", workers=4, staleness_bound=8, eval_every=0, **kw)
    return run_local(cfg, log=lambda *a, **k: None)["server"]


def test_lambda_zero_is_the_plain_apply(monkeypatch):
    """dc_lambda = 0: no delay_compensation record, and the run ends in the bits of the plain
    update — the same run with ParameterServer.apply replaced by the pre-DC body (dense wire ->
    apply_range) and the fetch bookkeeping by the bare core call."""
    got = _loopback()
    assert "delay_compensation" not in got and got["async_updates"] > 0

    def plain_apply(self, grads, weight, worker_id=None):
        self.apply_range(grads[: self.n], weight, 0, self.n)
        return self.finish_round_apply(-1.0)

    def plain_fetch(self, worker_id, dst=None):
        assert dst is None
        return self.core.on_fetch(worker_id)

    monkeypatch.setattr(ParameterServer, "apply", plain_apply)
    monkeypatch.setattr(ParameterServer, "note_fetch", plain_fetch)
    want = _loopback()
    assert got["final_param_sha256"] == want["final_param_sha256"]
    assert got["async_updates"] == want["async_updates"]


@pytest.mark.parametrize("adaptive", [False, True])
def test_run_local_async_with_dc(adaptive):
    srv = _loopback(dc_lambda=2.0 if adaptive else 0.04, dc_adaptive=adaptive)
    dc = srv["delay_compensation"]
    assert dc["adaptive"] is adaptive and dc["compensated_pushes"] > 0
    assert dc["compensated_pushes"] + dc["uncompensated_pushes"] == srv["async_updates"]
    assert np.isfinite(srv["final_param_checksum"])
