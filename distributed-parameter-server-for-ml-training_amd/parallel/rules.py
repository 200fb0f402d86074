"""The server's update rules: what ParameterServer.update_range (parallel/server.py) runs.

One rule per update form: SGD (momentum and weight decay included), LARS, AdamW, LAMB, and the
gradient guard, a wrapper that ends in the SGD rule. ``rule_of(cfg)`` picks the server's one rule.
A rule holds no state: it reads and writes the server it is handed (params, momentum_buf, adam_m /
adam_v / adam_t, agg, _lars_tab, _guard_state, ...). Its parts:

* ``whole``: the rule needs a norm over the whole arena before the first element moves, so the
  entry refuses a partial range with ``refusal``;
* ``adam``: the rule counts its updates in adam_t and keeps both moments (checkpoint / resume);
* ``table``: the rule keeps per-tensor ratios (the device segment table, ops/kernels.py LarsTable);
* ``scatters(cfg)``: a top-k payload may be scattered straight into the parameters;
* ``device_payload(s, codec, payloads, weight, img)``: the device form that decodes q8 / sign1
  payloads inside the update (the wrapper parallel/pushcodec.py names); None unless defined;
* ``device(s, srcs, weight, lo, hi, img, summed)``: the launches, through the wrappers of
  ops/kernels.py, always called as attributes of that module;
* ``host(s, srcs, weight, lo, hi, summed)``: the same formula in torch on a CPU arena; False when
  the round left the parameters alone;
* ``metrics(s)``: the rule's keys of final_metrics.

``srcs`` each hold params[lo:hi]'s gradient in their first hi - lo elements; ``summed``: the one
source already is the round's sum (apply_range), taken as is and not summed again.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops import kernels as K


def first_n(srcs: list, n: int) -> list:
    return [s if s.numel() == n else s[:n] for s in srcs]


def host_sum(srcs: list, n: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """The host forms' sum of the sources' first n elements: from zeros (``out``, or a new
    buffer), fixed order, fp32 accumulation."""
    out = torch.zeros(n, dtype=torch.float32, device=srcs[0].device) if out is None else out.zero_()
    for s in srcs:
        out.add_(s[:n].to(torch.float32))
    return out


def is_agg(s, srcs: list) -> bool:
    """The source is the server's aggregation buffer itself (a decoded or accumulated sum)."""
    return len(srcs) == 1 and srcs[0].dtype == torch.float32 and srcs[0].data_ptr() == s.agg.data_ptr()


def stage(s, srcs: list, name: str, *state, **kw):
    """How every whole-arena rule reaches its pair of kernel entries: the dense one
    (``K.<name>_apply``) when the source is the aggregation buffer, else the multi-source one
    (``K.<name>_apply_multi``), which leaves the sum there."""
    if is_agg(s, srcs):
        getattr(K, name + "_apply")(s.params, s.agg, *state, **kw)
    else:
        getattr(K, name + "_apply_multi")(s.params, first_n(srcs, s.n), s.agg, *state, **kw)


def stage_host(s, srcs: list):
    """The host form of ``stage``: the sum into the aggregation buffer unless it is the source."""
    if not is_agg(s, srcs):
        host_sum(srcs, s.n, out=s.agg)


def trust_ratios(s, kind, host_ratios):
    """{min, median, max} of the last update's per-tensor ratios over the adapted tensors (LARS:
    the trust ratio; LAMB: |w| / |u|), read from the device ratio table here, not per round; None
    before the first update, and on a server whose rule is not ``kind``."""
    if type(s.rule) is not kind or not s._ratios_applied:
        return None
    if s._lars_tab is not None:
        r = s._lars_tab.ratios.cpu()[torch.tensor(s._lars_tab.adapt)]
    else:
        r = torch.tensor(host_ratios)
    if not r.numel():
        return None
    return {"min": float(r.min()), "median": float(r.median()), "max": float(r.max())}


def _param_entries(s):
    return [e for e in s.layout.entries.values() if e.region == "param" and e.numel]


def _adam_hp(cfg) -> dict:
    return dict(beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_eps)


def _adam_metrics(s) -> dict:
    return {"beta1": float(s.cfg.adam_beta1), "beta2": float(s.cfg.adam_beta2), "eps": float(s.cfg.adam_eps),
            "steps": int(s.adam_t)}


def _scalars(fn: str, *a, **hp):
    try:
        return getattr(K, fn)(*a, **hp)
    except (OSError, RuntimeError, AttributeError):  # the kernel library is not loaded here
        return getattr(K, fn + "_host")(*a, **hp)


class Rule:
    """The parts of a rule that have a default (the module docstring lists them all)."""
    whole, adam, table, refusal = False, False, False, ""
    device_payload = None  # the in-kernel decode of q8 / sign1 payloads, where the rule has one

    def scatters(self, cfg) -> bool:
        return False

    def metrics(self, s) -> dict:
        return {}


class _SGDTail(Rule):
    """What the rules that end in the SGD tail share: its arguments, and its host form."""

    def _kw(self, s, weight, lo, hi, img) -> dict:
        return dict(gscale=weight, momentum=s.cfg.momentum, wd=s.cfg.weight_decay,
                    buf=s.momentum_buf[lo:hi] if s.momentum_buf is not None else None, first=s._mom_first,
                    n=hi - lo, img=img)

    def host(self, s, srcs, weight, lo, hi, summed):
        p = s.params[lo:hi]
        d = (srcs[0] if summed else host_sum(srcs, hi - lo)).to(torch.float32) * weight
        if s.cfg.weight_decay:
            d = d + s.cfg.weight_decay * p
        if s.momentum_buf is not None:
            buf = s.momentum_buf[lo:hi]
            if s._mom_first:
                buf.copy_(d)
            else:
                buf.mul_(s.cfg.momentum).add_(d)
            d = buf
        p.sub_(s.lr * d)


class SGD(_SGDTail):
    """p <- p - lr * (weight * g [+ wd p]) [momentum]: csrc/kernels/optim.hip (q8 / sign1
    payloads: csrc/kernels/q8.hip / sign1.hip, decoded inside the update). Element-wise: any range
    is legal, and the ranges of one round share the momentum 'first step' flag."""

    def scatters(self, cfg) -> bool:
        return not cfg.momentum and not cfg.weight_decay  # no optimizer state to keep in step

    def device(self, s, srcs, weight, lo, hi, img, summed):
        if summed:
            K.sgd_apply(s.params[lo:hi], srcs[0], s.lr, **self._kw(s, weight, lo, hi, img))
        else:
            K.sgd_apply_multi(s.params[lo:hi], first_n(srcs, hi - lo), s.lr, **self._kw(s, weight, lo, hi, img))

    def device_payload(self, s, codec, payloads, weight, img):
        getattr(K, codec.in_kernel)(s.params, payloads, s.lr, **self._kw(s, weight, 0, s.n, img))


class Guard(_SGDTail):
    """--clip-norm / --skip-nonfinite around the SGD rule: S = sum s^2 of the round's fp32 sum,
    norm = weight * sqrt(S); S not finite: the round is skipped (parameters, momentum buffer and
    fetch image untouched; it still counts as a round, and consumes the momentum 'first step' flag:
    the buffer starts as zeros, so momentum * 0 + d of the next round has the value the first-step
    form would have given); else coef = min(1, clip_norm / (norm + 1e-6)) (1 without --clip-norm),
    rounded to fp32, and the SGD update with weight * coef (one fp32 multiply): weight decay is
    added after the scaling, not clipped. Device: the three launches of csrc/kernels/gguard.hip, no
    host synchronisation, counters in the device state block; CPU arena: the same formula in torch
    (equal to a tolerance, not bit for bit: the reduction orders differ), counters in _guard_host."""
    whole = True
    refusal = ("--clip-norm / --skip-nonfinite need the whole gradient's norm before the first parameter moves: a "
               "partial range [{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)")

    def device(self, s, srcs, weight, lo, hi, img, summed):
        stage(s, srcs, "guard", s._guard_state, lr=s.lr, clip_norm=s.cfg.clip_norm, **self._kw(s, weight, lo, hi, img))

    def host(self, s, srcs, weight, lo, hi, summed):
        stage_host(s, srcs)
        S = float(s.agg.double().square().sum())
        h = s._guard_host
        h["rounds"] += 1
        if not math.isfinite(S):
            h["skipped_rounds"] += 1
            h["norm_last"] = float("nan") if S != S else float("inf")
            return False
        norm = float(np.float32(weight)) * math.sqrt(S)
        clip = s.cfg.clip_norm
        coef = np.float32(min(1.0, clip / (norm + 1e-6))) if clip > 0 else np.float32(1.0)
        h["clipped_rounds"] += int(coef < 1.0)
        h["norm_last"] = norm
        h["norm_max"] = max(h["norm_max"], norm)
        h["norm_sum"] += norm
        _SGDTail.host(self, s, [s.agg], float(np.float32(weight) * coef), lo, hi, True)

    def metrics(self, s) -> dict:
        return {"gradient_guard": s.guard_counters()}


class LARS(_SGDTail):
    """--optimizer lars: d = lambda_t * (weight * s + wd * w) for tensors with ndim > 1, lambda_t =
    trust * |w| / (weight * |s| + wd * |w| + eps) (1 when a norm is 0); d = weight * s for 1-D
    tensors; then the momentum form of SGD. Device: the two launches of csrc/kernels/lars.hip; CPU
    arena: the same formula in torch, tensor by tensor (equal to a tolerance, not bit for bit: the
    reduction orders differ)."""
    whole = table = True
    refusal = ("--optimizer lars needs every tensor's norm before its first element moves: a partial range "
               "[{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)")

    def device(self, s, srcs, weight, lo, hi, img, summed):
        s._ratios_applied = True
        stage(s, srcs, "lars", s._lars_tab, lr=s.lr, trust=s.cfg.lars_trust, eps=s.cfg.lars_eps,
              **self._kw(s, weight, lo, hi, img))

    def host(self, s, srcs, weight, lo, hi, summed):
        cfg = s.cfg
        s._ratios_applied = True
        stage_host(s, srcs)
        ratios = []
        for e in _param_entries(s):
            w = s.params[e.offset:e.offset + e.numel]
            d = s.agg[e.offset:e.offset + e.numel] * weight
            if len(e.shape) > 1:
                wn, gn = float(w.double().norm()), float(d.double().norm())
                lam = cfg.lars_trust * wn / (gn + cfg.weight_decay * wn + cfg.lars_eps) if wn > 0 and gn > 0 else 1.0
                ratios.append(lam)
                if cfg.weight_decay:
                    d = d + cfg.weight_decay * w
                d = d * lam
            if s.momentum_buf is not None:
                buf = s.momentum_buf[e.offset:e.offset + e.numel]
                if s._mom_first:
                    buf.copy_(d)
                else:
                    buf.mul_(cfg.momentum).add_(d)
                d = buf
            w.sub_(s.lr * d)
        s._lars_ratios = ratios

    def metrics(self, s) -> dict:
        return {"lars_trust_ratio": s.lars_trust_ratios()}


class AdamW(Rule):
    """--optimizer adamw, update number adam_t + 1: g = weight * s; m = beta1 m + (1 - beta1) g;
    v = beta2 v + (1 - beta2) g g; p = p (1 - lr wd) - lr / (1 - beta1^t) * m / (sqrt(v) /
    sqrt(1 - beta2^t) + eps). Element-wise: any range is legal, and every range of one round shares
    t. Device: one launch of csrc/kernels/adamw.hip; CPU arena: the same formula in torch fp32 from
    the same eight fp32 scalars (equal to a tolerance, not bit for bit)."""
    adam = True

    def device(self, s, srcs, weight, lo, hi, img, summed):
        K.adamw_apply_multi(s.params[lo:hi], first_n(srcs, hi - lo), s.adam_m[lo:hi], s.adam_v[lo:hi], s.lr,
                            s.adam_t + 1, gscale=weight, n=hi - lo, img=img, wd=s.cfg.weight_decay, **_adam_hp(s.cfg))

    def host(self, s, srcs, weight, lo, hi, summed):
        p, m, v = s.params[lo:hi], s.adam_m[lo:hi], s.adam_v[lo:hi]
        step_size, b1, omb1, b2, omb2, rbc2, eps, decay = _scalars("adamw_scalars", s.lr, s.adam_t + 1,
                                                                   wd=s.cfg.weight_decay, **_adam_hp(s.cfg))
        # plain element-wise fp32 ops only (no fused alpha forms): a range gives the whole round's bits
        g = host_sum(srcs, hi - lo) * float(np.float32(weight))
        m.copy_(m * b1 + g * omb1)
        v.copy_(v * b2 + (g * g) * omb2)
        den = v.sqrt() * rbc2 + eps
        p.copy_(p * decay - (m / den) * step_size)

    def metrics(self, s) -> dict:
        return {"adamw": _adam_metrics(s)}


class LAMB(AdamW):
    """--optimizer lamb (You et al. 2020), update number adam_t + 1: AdamW's g, m, v; r = m /
    (1 - beta1^t) / (sqrt(v) / sqrt(1 - beta2^t) + eps); tensors with ndim > 1: u = r + wd * w,
    phi = |w| / |u| (1 when a norm is 0); 1-D tensors: u = r, phi = 1; w -= lr * phi * u. No clamp
    on |w|, no global gradient normalisation. Device: the two launches of csrc/kernels/lamb.hip
    (the aggregation buffer ends holding u); CPU arena: the same formula in torch from the same
    fp32 scalars, tensor by tensor (equal to a tolerance, not bit for bit: the reduction orders
    differ)."""
    whole = table = True
    refusal = ("--optimizer lamb needs every tensor's norm before its first element moves: a partial range "
               "[{lo}, {hi}) of {n} cannot be applied (no bucketed or sharded updates)")

    def device(self, s, srcs, weight, lo, hi, img, summed):
        s._ratios_applied = True
        stage(s, srcs, "lamb", s.adam_m, s.adam_v, s._lars_tab, lr=s.lr, t=s.adam_t + 1, gscale=weight,
              wd=s.cfg.weight_decay, n=s.n, img=img, **_adam_hp(s.cfg))

    def host(self, s, srcs, weight, lo, hi, summed):
        s._ratios_applied = True
        stage_host(s, srcs)
        bc1, b1, omb1, b2, omb2, rbc2, eps, _ = _scalars("lamb_scalars", s.adam_t + 1, **_adam_hp(s.cfg))
        lr, wd = float(np.float32(s.lr)), float(np.float32(s.cfg.weight_decay))
        g = s.agg * float(np.float32(weight))
        s.adam_m.copy_(s.adam_m * b1 + g * omb1)
        s.adam_v.copy_(s.adam_v * b2 + (g * g) * omb2)
        r = (s.adam_m / (s.adam_v.sqrt() * rbc2 + eps)) * bc1
        ratios = []
        for e in _param_entries(s):
            w = s.params[e.offset:e.offset + e.numel]
            u = r[e.offset:e.offset + e.numel]
            phi = 1.0
            if len(e.shape) > 1:
                u = u + wd * w
                wn, un = float(w.double().norm()), float(u.double().norm())
                phi = float(np.float32(wn / un)) if wn > 0 and un > 0 else 1.0
                ratios.append(phi)
            w.sub_(float(np.float32(lr * phi)) * u)
        s._lamb_ratios = ratios

    def metrics(self, s) -> dict:
        return {"lamb": _adam_metrics(s), "lamb_trust_ratio": s.lamb_trust_ratios()}


_OPTIMIZERS = {"sgd": SGD(), "lars": LARS(), "adamw": AdamW(), "lamb": LAMB()}
_GUARD = Guard()


def rule_of(cfg):
    """The one rule of a server with this configuration (the guard runs on the SGD update only:
    utils/config.py validates that)."""
    return _GUARD if cfg.grad_guard else _OPTIMIZERS[cfg.optimizer]
