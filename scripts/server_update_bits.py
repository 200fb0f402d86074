#!/usr/bin/env python
"""Fingerprints of the server update on every route: one line per (rule, entry, update) with the
sha256 of everything an update may write.

Drives a fresh ParameterServer (resnet_tiny's layout, weight wire enabled) through three updates
of seeded gradients for every update rule crossed with every public routing method that the
rule's configuration admits, and prints after each update the hashes of the arena, the momentum
buffer, both Adam moments and the wire image, the stale flag, the guard counters, adam_t and the
global step. Two runs of the same code on the same device print the same lines; a refactor of the
routing prints the lines of its parent (profiles/server_rules_bits.txt holds both).

    python scripts/server_update_bits.py --device cpu|cuda

Gradients, q8 and top-k payloads are made on the host from one seed and copied to the device, so
both devices are fed the same bytes. The three rounds are scaled 0.01, 0.16, 0.01: a clip bound
between the two magnitudes clips the second round and only that.
"""
import argparse
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.models.layout import ParamLayout  # noqa: E402
from psx.models.resnet import TinyResNet  # noqa: E402
from psx.parallel import q8 as Q  # noqa: E402
from psx.parallel import topk as T  # noqa: E402
from psx.parallel.server import ParameterServer  # noqa: E402
from psx.utils.config import PSConfig  # noqa: E402

ROUNDS, W = 3, 3
SCALES = [0.01, 0.16, 0.01]
TOPK_RATIO = 0.25

RULES = {  # name -> PSConfig fields
    "sgd": {},
    "sgd_mom_wd": dict(momentum=0.9, weight_decay=5e-4),
    "lars": dict(optimizer="lars", momentum=0.9, weight_decay=5e-4),
    "adamw": dict(optimizer="adamw", weight_decay=0.01),
    "lamb": dict(optimizer="lamb", weight_decay=0.01),
    "guard_clip": dict(clip_norm=-1.0, momentum=0.9, weight_decay=5e-4),  # the bound is set per entry
    "guard_inf": dict(skip_nonfinite=True, momentum=0.9),
    "dc": dict(mode="async", dc_lambda=0.04, momentum=0.9, weight_decay=5e-4),
    "dc_adaptive": dict(mode="async", dc_lambda=0.04, dc_adaptive=True),
}
ELEMENTWISE = ("sgd", "sgd_mom_wd", "adamw")
DC = ("dc", "dc_adaptive")
ENTRIES = ("apply_fp16", "apply_fp32", "apply_q8", "apply_topk", "sources3_fp16", "range_sources_whole",
           "range_sources_uneven", "push_loopback2")


def sha(t) -> str:
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def admits(rule: str, entry: str) -> bool:
    if entry == "range_sources_uneven":
        return rule in ELEMENTWISE
    if rule in DC:  # async pushes only
        return entry.startswith("apply_") or entry == "push_loopback2"
    if rule == "guard_inf":  # the non-finite value travels in a dense wire
        return entry not in ("apply_q8", "apply_topk")
    return True


def gradients(n: int):
    gen = torch.Generator().manual_seed(1234)
    return [[torch.randn(n, generator=gen) * sc for _ in range(W)] for sc in SCALES]


def make_server(rule: str, entry: str, lay, arena, counters, device, G):
    kw = dict(model="resnet_tiny", batch_size=8, epochs=1, train_samples=96, test_samples=32, verbose=0,
              use_graph=False, lr=0.05, mode="sync", topk_ratio=TOPK_RATIO)
    kw.update(RULES[rule])
    workers = 2 if entry == "push_loopback2" else 1 if entry.startswith("apply_") else W
    if entry.startswith("apply_") and rule not in DC:
        kw["mode"] = "async"
    kw["workers"] = workers
    kw["codec"] = {"apply_fp32": "none", "apply_q8": "q8", "apply_topk": "topk"}.get(entry, "fp16")
    if rule == "guard_clip":  # between the norms of the small and the large rounds' weighted sums
        k = 1 if entry.startswith("apply_") else workers
        norms = [float(sum(g[:k]).double().norm()) / k for g in G]
        kw["clip_norm"] = math.sqrt(norms[0] * norms[1])
    cfg = PSConfig(**kw).validate()
    s = ParameterServer(cfg, lay, arena.clone(), counters.clone(), device=device, total_workers=workers,
                        log=lambda *a, **k: None)
    for w in range(workers):
        s.register_worker(f"w{w}", w)
    s.enable_weight_wire()
    return s


def run_cell(rule: str, entry: str, lay, arena, counters, device, G):
    n = lay.param_numel
    s = make_server(rule, entry, lay, arena, counters, device, G)
    q8enc, tkenc = Q.Q8Codec(n, "cpu"), T.TopKCodec(n, TOPK_RATIO, "cpu")
    for r in range(ROUNDS):
        g = [x.clone() for x in G[r]]
        if rule == "guard_inf" and r == 1:
            g[0][7] = float("inf")
        h = [x.half().to(device) for x in g]
        if rule in DC and r > 0:  # the first push finds no backup, the later ones are compensated
            for w in range(s.total_workers):
                s.fetch_parameters(w)
        if entry == "apply_fp16":
            s.apply(h[0], 0.5, 0)
        elif entry == "apply_fp32":
            s.apply(g[0].to(device), 0.5, 0)
        elif entry == "apply_q8":
            q8enc.resid.zero_()
            s.apply(q8enc.encode(g[0]).clone().to(device), 0.5, 0)
        elif entry == "apply_topk":
            tkenc.resid.zero_()
            s.apply(tkenc.encode(g[0]).clone().to(device), 0.5, 0)
        elif entry == "sources3_fp16":
            assert s.apply_sources(h, [0, 1, 2], [s.core.global_step] * 3)
        elif entry == "range_sources_whole":
            s.apply_range_sources(h, 1.0 / W, 0, n)
            s.finish_round_apply()
        elif entry == "range_sources_uneven":
            cuts = [0, n // 3 + 1, 2 * n // 3 + 3, n]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                s.apply_range_sources(h, 1.0 / W, lo, hi)
            s.finish_round_apply()
        else:  # push_loopback2
            for w in range(2):
                s.push_gradients(w, h[w], s.core.global_step)
        gc = s.guard_counters()
        guard = "-" if gc is None else hashlib.sha256(json.dumps(gc, sort_keys=True).encode()).hexdigest()[:16]
        print(f"{rule} {entry} u{r + 1} arena={sha(s.arena)} mom={sha(s.momentum_buf)} m={sha(s.adam_m)} "
              f"v={sha(s.adam_v)} img={sha(s.wire.img)} stale={int(s._wire_stale)} guard={guard} "
              f"adam_t={s.adam_t} gs={s.core.global_step}", flush=True)
    updates = ROUNDS * 2 if rule in DC and entry == "push_loopback2" else ROUNDS  # an async push is an update
    assert s.core.global_step == updates, (rule, entry, s.core.global_step)
    if rule == "guard_clip":
        assert gc["clipped_rounds"] >= 1 and gc["skipped_rounds"] == 0, (entry, gc)
    if rule == "guard_inf":
        assert gc["skipped_rounds"] == 1, (entry, gc)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", choices=["cpu", "cuda"], default="cpu")
    device = ap.parse_args(argv).device
    torch.manual_seed(2)
    model = TinyResNet(10)
    lay = ParamLayout.from_module(model)
    arena, counters = lay.pack(model)
    G = gradients(lay.param_numel)
    cells = 0
    for rule in RULES:
        for entry in ENTRIES:
            if admits(rule, entry):
                run_cell(rule, entry, lay, arena, counters, device, G)
                cells += 1
    if device == "cuda":
        torch.cuda.synchronize()
    print(f"# {cells} cells of {ROUNDS} rounds, device {device}", flush=True)


if __name__ == "__main__":
    main()
