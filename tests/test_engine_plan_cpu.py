"""The engine's step plan (models/plan.py plan_step) against a golden table. Host code only: runs
without a GPU.

tests/golden/engine_plans.json holds one record per configuration: ResNet-18 / CIFAR at batches 8,
32, 128 in fp32 and bf16 under the options default, wgrad_stream=1, wino=0, wino_bwdfold=0,
wino_bnfold=0, wgrad_rbatch=0 (bn_finalize "apply"), one bn_finalize="conv" row (with fuse_bnbwd
off, as tests/test_engine_gpu.py runs that mode) and one "separate" row (bf16, batch 32), and
ResNet-50 / 224 at batches 16 and 64 in fp32 and bf16 with default options: 42 records. Every
record was read off the engine of the commit before plan.py existed, on an MI355X, after one eager
training step: its name-keyed route sets, the sets it filled while issuing the step (folds, late
weight transforms, the tail weight gradient), the refusals its launches returned (stem, shortcut
fold, head sums) and its buffer sizes. So the table pins the plan across that refactor. Layer rows
are stored once per distinct table (``conv_tables`` / ``bn_tables``, rows under ``*_columns`` in
``names`` order) and referenced by index; the BN slot offsets (``slots``) depend on the model alone."""
import json
import os
from dataclasses import replace

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_plans.json")
R18_TUNES = [{}, {"wgrad_stream": "1"}, {"wino": "0"}, {"wino_bwdfold": "0"}, {"wino_bnfold": "0"},
             {"wgrad_rbatch": "0"}]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _key(c):
    return (c["model"], c["batch"], c["f32"], tuple(sorted(c["tune"].items())), c["bn_finalize"], c["fuse_bnbwd"])


def test_golden_table_configurations():
    """The table holds exactly the configurations the docstring names."""
    want = [("resnet18", B, f32, tuple(sorted(t.items())), "apply", True)
            for B in (8, 32, 128) for f32 in (True, False) for t in R18_TUNES]
    want += [("resnet18", 32, False, (), "conv", False), ("resnet18", 32, False, (), "separate", True)]
    want += [("resnet50", B, f32, (), "apply", True) for B in (16, 64) for f32 in (True, False)]
    got = [_key(r["config"]) for r in _golden()["records"]]
    assert len(got) == len(set(got)) == 42
    assert sorted(got) == sorted(want)
    assert all(r["config"]["deterministic"] and r["config"]["in_hw"] == (224 if r["config"]["model"] == "resnet50"
                                                                        else 32) for r in _golden()["records"])


@pytest.fixture(scope="module")
def specs():
    from psx.models.plan import netspec_from_module
    from psx.models.resnet import ResNet18, ResNet50

    models = {"resnet18": (ResNet18(100), (32, 32)), "resnet50": (ResNet50(1000), (224, 224))}
    return {(m, f32): netspec_from_module(mod, hw, f32) for m, (mod, hw) in models.items() for f32 in (True, False)}


def _enc(v, none):
    """A plan field as the table stores it: booleans as 0 / 1, no route as ``none``."""
    return none if v is None else int(v) if isinstance(v, bool) else v


def _plan(cfg, spec, monkeypatch):
    from psx.models.plan import EngineOptions, plan_step

    monkeypatch.setenv("PSX_TUNE", ",".join(f"{k}={v}" for k, v in cfg["tune"].items()))
    opts = replace(EngineOptions.from_env(cfg["f32"], spec.in_hw, cfg["deterministic"]),
                   bn_finalize=cfg["bn_finalize"], fuse_bnbwd=cfg["fuse_bnbwd"])
    return plan_step(spec, cfg["batch"], cfg["f32"], opts)


def test_plan_reproduces_golden(specs, monkeypatch):
    g = _golden()
    bad = []
    for rec in g["records"]:
        cfg = rec["config"]
        plan = _plan(cfg, specs[cfg["model"], cfg["f32"]], monkeypatch)
        names = g["names"][cfg["model"]]
        assert list(plan.convs) == names["convs"] and list(plan.bns) == names["bns"]
        got_c = [[_enc(getattr(p, k), "none") for k in g["conv_columns"]] for p in plan.convs.values()]
        got_b = [[_enc(getattr(p, k), None) for k in g["bn_columns"]] for p in plan.bns.values()]
        got_s = [[getattr(p, k) for k in g["slot_columns"]] for p in plan.bns.values()]
        wino = bool(plan.wino_names())  # the Winograd scratch exists only in an engine with such layers
        got_t = dict(wbuf=plan.wbuf, wpart=max(1, plan.wpart), wpart_w=max(1, plan.wpart_w),
                     s_main=max(1, plan.s_main) if wino else 0, s_d=max(1, plan.s_d) if wino else 0,
                     s_part=max(1, plan.s_part) if wino else 0,
                     red_len=plan.red_len, ctr_words=plan.ctr_words, nshift=plan.nshift,
                     tail_split=int(plan.tail_split), wgrad_stream=int(plan.wgrad_stream), late=sorted(plan.late_names()),
                     bnfold=plan.bnfold)
        want_t = {k: v for k, v in rec["totals"].items() if k not in ("ntiles", "ndesc")}
        for what, got, want in (("convs", got_c, g["conv_tables"][rec["convs"]]), ("bns", got_b, g["bn_tables"][rec["bns"]]),
                                ("slots", got_s, g["slots"][cfg["model"]]), ("totals", got_t, want_t)):
            if got != want:
                rows = [(n, a, b) for n, a, b in zip(names[what] if what in names else names["bns"], got, want)
                        if a != b] if what != "totals" else [(k, got[k], want[k]) for k in want if got.get(k) != want[k]]
                bad.append((_key(cfg), what, rows[:4]))
    assert not bad, bad[:6]


def test_options_from_env(monkeypatch):
    """EngineOptions.from_env: the defaults, the "auto" side-stream rule and each PSX_TUNE key."""
    from psx.models.plan import EngineOptions

    monkeypatch.delenv("PSX_TUNE", raising=False)
    monkeypatch.delenv("PSX_DETERMINISTIC", raising=False)
    d = EngineOptions.from_env(True, (32, 32))
    assert d == EngineOptions(wgrad_stream=False) and d.deterministic and d.bn_finalize == "apply" and d.bwd_fold == "all"
    assert EngineOptions.from_env(False, (32, 32)).wgrad_stream and EngineOptions.from_env(True, (224, 224)).wgrad_stream
    monkeypatch.setenv("PSX_DETERMINISTIC", "0")
    assert not EngineOptions.from_env(True, (32, 32)).deterministic
    assert EngineOptions.from_env(True, (32, 32), deterministic=True).deterministic
    monkeypatch.setenv("PSX_TUNE", "wgrad_stream=1,wino=0,wino_bwdfold=0,wino_bnfold=0,wgrad_rbatch=0")
    o = EngineOptions.from_env(True, (32, 32))
    assert (o.wgrad_stream, o.wino, o.bwd_fold, o.wino_bnfold, o.wgrad_rbatch) == (True, False, "off", False, False)
    with pytest.raises(AssertionError):
        EngineOptions(bn_finalize="fused")


def test_stem_and_head_queries():
    """The host queries lifted out of the stem and head entries answer the entries' own shape tests."""
    from psx.ops import kernels as K

    assert K.stem_ok(8, 32, 32, 3, 4, 64, 64, True) and K.stem_ok(8, 32, 32, 3, 8, 64, 128, False)
    assert not K.stem_ok(8, 32, 32, 3, 8, 64, 64, True)       # cp of the other dtype
    assert not K.stem_ok(8, 32, 30, 3, 4, 64, 64, True)       # W % 4
    assert K.stem_ok(4, 224, 224, 3, 4, 64, 196, True, k=7) and K.stem_ok(4, 224, 224, 3, 8, 64, 448, False, k=7)
    assert not K.stem_ok(4, 112, 112, 3, 4, 64, 196, True, k=7)
    assert K.head_sums_ok(512, 100) and not K.head_sums_ok(2048, 1000)  # the large head takes the split path
    assert not K.head_sums_ok(520, 100)                       # refused by the fused head (C % 16)
