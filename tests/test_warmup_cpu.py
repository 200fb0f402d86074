"""--warmup-steps N on the CPU path: update k (1-based) runs with lr * min(1, k / N). The lr
sequence, servers with warmup against servers whose lr is set by hand before every update (bit
for bit), resume in the middle of the warmup, and the paths that hold a fixed lr and decline."""
import types

import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

from .test_ps_cpu import tiny_cfg

BASE = 0.05


def lr_of(k: int, n: int, base: float = BASE) -> float:
    return base * min(1.0, k / n)


def tiny_server(device="cpu", **kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(**{**dict(mode="async", workers=1, lr=BASE, codec="none"), **kw})
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=1, log=lambda *a: None)
    s.register_worker("w", 0)
    return s, lay


def grads(n, count, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * 1e-2 for _ in range(count)]


def test_config():
    assert PSConfig().validate().warmup_steps == 0
    assert PSConfig(warmup_steps=3).validate().warmup_steps == 3
    with pytest.raises(ValueError, match="--warmup-steps"):
        PSConfig(warmup_steps=-1).validate()
    from psx.utils.config import parse

    assert parse(["--warmup-steps", "12"]).warmup_steps == 12 and parse([]).warmup_steps == 0


def test_lr_sequence():
    s, lay = tiny_server(warmup_steps=5)
    seen = []
    for g in grads(lay.param_numel, 8):
        seen.append(s.lr)
        s.apply(g, 1.0)
    assert seen == [lr_of(k, 5) for k in range(1, 9)]
    assert seen[:5] == pytest.approx([0.01, 0.02, 0.03, 0.04, 0.05], rel=1e-15) and seen[4:] == [BASE] * 4
    fm = s.final_metrics()
    assert fm["warmup_steps"] == 5 and fm["effective_lr"] == BASE
    off, _ = tiny_server()
    assert off.lr == BASE and "effective_lr" not in off.final_metrics()


def test_rejected_push_advances_nothing():
    """An async push the staleness bound rejects is not applied: the count, and the lr, stay."""
    s, lay = tiny_server(workers=2, warmup_steps=4, staleness_bound=0)
    s.register_worker("w", 1)
    g = grads(lay.param_numel, 1)[0]
    s.fetch_parameters(0)
    s.fetch_parameters(1)
    assert s.lr == lr_of(1, 4)
    assert s.push_gradients(0, g, 0)  # computed at version 0
    assert s.lr == lr_of(2, 4)
    before = s.arena.clone()
    assert not s.push_gradients(1, g, 0)  # version 0 again: staleness 1 > bound 0
    assert s.lr == lr_of(2, 4) and s.core.global_step == 1 and torch.equal(s.arena, before)


@pytest.mark.parametrize("opt", [dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4),
                                 dict(optimizer="adamw", weight_decay=1e-2),
                                 dict(optimizer="lars", momentum=0.9, weight_decay=5e-4),
                                 dict(optimizer="lamb", weight_decay=1e-2)],
                         ids=["sgd", "adamw", "lars", "lamb"])
def test_warmup_equals_lr_set_by_hand(opt):
    a, lay = tiny_server(warmup_steps=4, **opt)
    b, _ = tiny_server(**opt)
    for k, g in enumerate(grads(lay.param_numel, 6), start=1):
        b.lr = lr_of(k, 4)
        assert a.lr == b.lr
        a.apply(g, 0.5)
        b.apply(g, 0.5)
        assert torch.equal(a.arena, b.arena), k
    if a.adam_m is not None:
        assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    c, _ = tiny_server(**opt)  # and the warmup changed something
    for g in grads(lay.param_numel, 6):
        c.apply(g, 0.5)
    assert not torch.equal(a.arena, c.arena)


def test_resume_in_the_middle(tmp_path):
    kw = dict(warmup_steps=6, ckpt_dir=str(tmp_path), momentum=0.9)
    a, lay = tiny_server(**kw)
    gs = grads(lay.param_numel, 5)
    for g in gs[:2]:
        a.apply(g, 1.0)
    path = a.checkpoint()
    for g in gs[2:]:
        a.apply(g, 1.0)
    b, _ = tiny_server(**kw)
    b.resume(path)
    assert b.core.global_step == 2 and b.lr == lr_of(3, 6)
    for g in gs[2:]:
        b.apply(g, 1.0)
    assert torch.equal(a.arena, b.arena) and a.lr == b.lr == lr_of(6, 6)


def test_fixed_lr_paths_decline(monkeypatch):
    """The native event loop, the native sync loop and the graph round hold the lr they were
    started with: off with N > 0 (their classes raise), unchanged with N = 0."""
    from psx.parallel.graph_round import GraphRoundChannel, graph_round_enabled
    from psx.parallel.native_loop import NativeServerLoop, native_loop_enabled
    from psx.parallel.native_sync import NativeSyncServer, native_sync_enabled
    from psx.parallel.runner import run_local_threads
    from psx.parallel.worker import SyncCollectiveChannel

    for k in ("PSX_NATIVE_LOOP", "PSX_NATIVE_SYNC", "PSX_SYNC_AGG"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PSX_GRAPH_ROUND", "1")
    t = types.SimpleNamespace(native=True, world_size=3, rank=0)
    srv = types.SimpleNamespace(wire=None)
    for n, want in ((0, True), (3, False)):
        a = PSConfig(mode="async", warmup_steps=n).validate()
        assert native_loop_enabled(a, t) is want
        s = PSConfig(mode="sync", topology="dedicated", warmup_steps=n).validate()
        chan = SyncCollectiveChannel(t, srv, members=[0, 1], codec=None, root_worker=False)
        assert native_sync_enabled(s, t, chan, srv, 0) is want
        c = PSConfig(mode="sync", topology="colocated", warmup_steps=n).validate()
        assert graph_round_enabled(c, t) is want
    w = PSConfig(mode="async", warmup_steps=3).validate()
    stub = types.SimpleNamespace(cfg=w, layout=None, device="cpu")
    with pytest.raises(ValueError, match="--warmup-steps"):
        NativeServerLoop(stub, None, None, {}, 1)
    with pytest.raises(ValueError, match="--warmup-steps"):
        NativeSyncServer(stub, t, None)
    with pytest.raises(ValueError, match="--warmup-steps"):
        GraphRoundChannel(t, stub, [0, 1], None, None, [], "cpu")
    with pytest.raises(ValueError, match="--warmup-steps"):
        run_local_threads(w, 1)
