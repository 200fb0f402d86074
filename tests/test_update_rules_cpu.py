"""ParameterServer.update_range, the one entry every route ends in, and the update rules of
parallel/rules.py behind it, on a CPU arena (tests/test_update_rules_gpu.py runs the same checks on
a device arena): a round in uneven ranges against the whole range, bit for bit; the refusal of a
partial range by every whole-arena rule, with nothing written; an image of the caller's; and every
public routing method under every rule. resnet_tiny's layout."""
import re

import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel import q8 as Q
from psx.parallel import topk as T
from psx.parallel.server import ParameterServer

from .test_ps_cpu import tiny_cfg

W = 3
RULES = {
    "sgd": {},
    "sgd_mom_wd": dict(momentum=0.9, weight_decay=5e-4),
    "adamw": dict(optimizer="adamw", weight_decay=0.01),
    "lars": dict(optimizer="lars", momentum=0.9, weight_decay=5e-4),
    "lamb": dict(optimizer="lamb", weight_decay=0.01),
    "guard": dict(clip_norm=0.05, momentum=0.9),
}
ELEMENTWISE = ("sgd", "sgd_mom_wd", "adamw")
WHOLE = ("lars", "lamb", "guard")
REFUSAL = {
    "lars": "--optimizer lars needs every tensor's norm before its first element moves: a partial range "
            "[{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)",
    "lamb": "--optimizer lamb needs every tensor's norm before its first element moves: a partial range "
            "[{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)",
    "guard": "--clip-norm / --skip-nonfinite need the whole gradient's norm before the first parameter moves: a "
             "partial range [{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)",
}


def make_server(rule, device, workers=W, **kw):
    torch.manual_seed(2)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(**{**dict(mode="sync", workers=workers, codec="fp16", topk_ratio=0.25), **RULES[rule], **kw})
    s = ParameterServer(cfg, lay, arena.clone(), counters, device=device, total_workers=workers, log=lambda *a: None)
    for w in range(workers):
        s.register_worker(f"w{w}", w)
    s.enable_weight_wire()
    return s, lay.param_numel


def dense_grads(n, rounds, count=W, seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=gen) * 1e-2 for _ in range(count)] for _ in range(rounds)]


def state_of(s):
    """Everything an update may write, as comparable values."""
    t = {k: None if v is None else v.detach().clone().cpu() for k, v in dict(
        params=s.params, mom=s.momentum_buf, m=s.adam_m, v=s.adam_v, agg=s.agg,
        img=s.wire.img.view(torch.int16)).items()}
    t.update(adam_t=s.adam_t, global_step=s.core.global_step, guard=s.guard_counters(), stale=s._wire_stale)
    return t


def assert_same_state(a, b, keys=None):
    for k in keys or a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert y is not None and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                 y.view(torch.int32) if y.dtype == torch.float32 else y), k
        elif isinstance(x, dict):  # guard counters: norm_last may be NaN
            assert repr(x) == repr(y), k
        else:
            assert x == y, k


def uneven_cuts(n):
    """Three ranges whose inner bounds are no multiple of 8: the vector kernels' head and tail lanes run."""
    return [0, n // 3 + 1, 2 * n // 3 + 3, n]


# ---------------------------------------------------------------------------- the checks (device-independent)
def check_ranges_give_the_whole_rounds_bits(rule, device):
    a, n = make_server(rule, device)
    b, _ = make_server(rule, device)
    cuts = uneven_cuts(n)
    assert cuts[1] % 8 and cuts[2] % 8
    for wires in dense_grads(n, 2):  # the second round runs the momentum form and t = 2
        srcs = [g.half().to(device) for g in wires]
        a.update_range(srcs, 1.0 / W, 0, n)
        a.finish_round_apply()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            b.update_range([s[lo:hi] for s in srcs], 1.0 / W, lo, hi)
        b.finish_round_apply()
        a.wire_for_fetch(), b.wire_for_fetch()
        assert_same_state(state_of(a), state_of(b), ("params", "mom", "m", "v", "img", "adam_t", "global_step"))
    assert a.core.global_step == 2 and a.adam_t == (2 if rule == "adamw" else 0)
    assert torch.equal(a.wire.img, a.params.bfloat16())


def check_partial_range_is_refused(rule, device):
    s, n = make_server(rule, device)
    srcs = [g.half().to(device) for g in dense_grads(n, 1)[0]]
    s.update_range(srcs, 1.0 / W, 0, n)  # one real update first: moments, agg and counters are not zeros
    s.finish_round_apply()
    before = state_of(s)
    for lo, hi in ((0, n - 1), (1, n), (8, 16)):
        text = re.escape(REFUSAL[rule].format(lo=lo, hi=hi, n=n))
        with pytest.raises(ValueError, match=text):
            s.update_range([x[lo:hi] for x in srcs], 1.0 / W, lo, hi)
        with pytest.raises(ValueError, match=text):
            s.apply_range(srcs[0][lo:hi], 1.0, lo, hi)
        with pytest.raises(ValueError, match=text):
            s.apply_range_sources(srcs, 1.0 / W, lo, hi)
    assert_same_state(before, state_of(s))


def check_image_of_the_caller(rule, device):
    """The sharded server's case: the entry writes the image slice it is handed, not the wire's."""
    s, n = make_server(rule, device)
    lo, hi = (0, n) if rule in WHOLE else (n // 3 + 1, 2 * n // 3 + 3)
    srcs = [g.half().to(device)[lo:hi] for g in dense_grads(n, 1)[0]]
    own = torch.zeros(hi - lo, dtype=torch.bfloat16, device=device)
    wire_img, p_old = s.wire.img.clone(), s.params.clone()
    s.update_range(srcs, 1.0 / W, lo, hi, img=own)
    s.finish_round_apply()
    assert not torch.equal(p_old[lo:hi], s.params[lo:hi])
    assert torch.equal(own, s.params[lo:hi].bfloat16())
    assert torch.equal(s.wire.img.view(torch.int16), wire_img.view(torch.int16)) and s._wire_stale
    assert torch.equal(s.wire_for_fetch().img, s.params.bfloat16())


def _payloads(n, wires, kind, device):
    out = []
    for g in wires:
        enc = Q.Q8Codec(n, "cpu") if kind == "q8" else T.TopKCodec(n, 0.25, "cpu")
        out.append(enc.encode(g).clone().to(device))
    return out


ROUTES = ("apply", "apply_range", "apply_range_sources", "apply_sources", "apply_reduced", "apply_gathered",
          "apply_payload_sources", "_apply_payloads", "push_gradients")


def check_every_route_updates(rule, device):
    """One server per routing method: the call is an update under this rule (the global step
    advanced, the parameters moved, adam_t advanced where the rule counts it)."""
    members, steps = list(range(W)), [0] * W
    for route in ROUTES:
        s, n = make_server(rule, device)
        wires = dense_grads(n, 1)[0]
        h = [g.half().to(device) for g in wires]
        p_old = s.params.clone()
        if route == "apply":
            s.apply(h[0], 1.0)
        elif route == "apply_range":
            s.apply_range(wires[0].to(device), 1.0, 0, n)
            s.finish_round_apply()
        elif route == "apply_range_sources":
            s.apply_range_sources(h, 1.0 / W, 0, n)
            s.finish_round_apply()
        elif route == "apply_sources":
            assert s.apply_sources(h, members, steps)
        elif route == "apply_reduced":
            assert s.apply_reduced(sum(wires).to(device), members, steps)
        elif route == "apply_gathered":
            assert s.apply_gathered(_payloads(n, wires, "topk", device), members, steps)
        elif route == "apply_payload_sources":
            assert s.apply_payload_sources(_payloads(n, wires, "q8", device), members, steps)
        elif route == "_apply_payloads":
            s._apply_payloads(_payloads(n, wires, "q8", device), 1.0 / W)
            s.finish_round_apply()
        else:
            for w in members:
                s.push_gradients(w, h[w], 0)
        assert s.core.global_step == 1, (rule, route)
        assert not torch.equal(p_old, s.params) and bool(torch.isfinite(s.params).all()), (rule, route)
        assert s.adam_t == (1 if rule in ("adamw", "lamb") else 0), (rule, route)
        if rule == "guard":
            assert s.guard_counters()["rounds"] == 1, route
        assert torch.equal(s.wire_for_fetch().img, s.params.bfloat16()), (rule, route)


# ---------------------------------------------------------------------------- CPU arena
@pytest.mark.parametrize("rule", ELEMENTWISE)
def test_ranges_give_the_whole_rounds_bits(rule):
    check_ranges_give_the_whole_rounds_bits(rule, "cpu")


@pytest.mark.parametrize("rule", WHOLE)
def test_partial_range_is_refused(rule):
    check_partial_range_is_refused(rule, "cpu")


@pytest.mark.parametrize("rule", list(RULES))
def test_image_of_the_caller(rule):
    check_image_of_the_caller(rule, "cpu")


@pytest.mark.parametrize("rule", list(RULES))
def test_every_route_updates(rule):
    check_every_route_updates(rule, "cpu")
