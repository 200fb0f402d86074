"""Timing of the iterative robust-aggregation kernels (csrc/kernels/robust_iter.hip).

  python bench/robust_iter_bench.py [--model resnet18] [--workers 3,7,15,31] [--iters 3] [--groups 20]
                                    [--per-group 10]

On the model's trainable size, W fp16 wires, for geomed and cclip: the device time of a whole round
(INIT, weights, (MID, weights) x (L - 1), LAST: 2 L + 1 launches) and of one MID pass alone, in one
process, the kernels taking turns, cache-warm and after a cache scrub (bench/q8_bench.py for the two
schemes). Yardsticks, timed beside them:
  sgd_apply_multi with the same W (no momentum, no image): one read of the same wires plus 4 read and 4
    written per element;
  a streaming fp32 copy moving the same number of bytes. A pass reads 2 W per element; cclip adds 4
    read and 4 written (the centre; INIT only reads it); LAST adds 4 for agg. The weight steps and the
    partials are not counted: the round's time carries them, the bytes do not.
The expectation is time <= 1.10 x the copy of equal bytes; a cell above it is marked MISS with its
ratio. Nothing is gated on it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import psx  # noqa: E402,F401
from bench.q8_bench import time_alternating  # noqa: E402
from psx.models.layout import ParamLayout  # noqa: E402
from psx.models.resnet import build_model  # noqa: E402
from psx.ops import kernels as K  # noqa: E402


def round_of(wires, st, rule, L, agg, tau):
    """One round as Robust.combine issues it."""
    W = len(wires)
    K.robust_iter_step(wires, st, "init")
    for t in range(L):
        K.robust_iter_weights(st, W, rule, tau=tau, final=t == L - 1)
        if t < L - 1:
            K.robust_iter_step(wires, st, "mid")
    K.robust_iter_step(wires, st, "last", agg=agg, c=float(W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--workers", default="3,7,15,31")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    a = ap.parse_args()
    dev, L = "cuda", a.iters
    n = ParamLayout.from_module(build_model(a.model, 100)).param_numel
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    print(f"{a.model}: n = {n}, L = {L}", flush=True)
    agg, p = torch.zeros(n, device=dev), torch.randn(n, device=dev) * 0.05
    states = {"geomed": K.RobustIterState(n, dev), "cclip": K.RobustIterState(n, dev, centre=True)}
    misses = []
    for W in [int(w) for w in a.workers.split(",")]:
        wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
        tau = 0.5 * float(wires[0].float().norm())  # every wire is clipped: b stays away from 0 and 1
        fns = {"sgd_apply_multi": lambda: K.sgd_apply_multi(p, wires, 1e-6, gscale=1.0 / W, n=n)}
        nbytes = {}
        for rule, st in states.items():
            cb = 8 if rule == "cclip" else 0
            nbytes[f"{rule} round"] = n * ((L + 1) * 2 * W + L * cb + cb // 2 + 4)
            nbytes[f"{rule} mid"] = n * (2 * W + cb)
            fns[f"{rule} round"] = lambda rule=rule, st=st: round_of(wires, st, rule, L, agg, tau)
            fns[f"{rule} mid"] = lambda st=st: K.robust_iter_step(wires, st, "mid")  # with the round's last weights
        for k, b in nbytes.items():
            src, dst = torch.zeros(b // 8, device=dev), torch.zeros(b // 8, device=dev)
            fns[f"copy ({k})"] = lambda src=src, dst=dst: dst.copy_(src)
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            t = time_alternating(fns, a.groups, a.per_group, scrub)
            for k, b in nbytes.items():
                cp = t[f"copy ({k})"]
                ratio = t[k] / cp
                ok = ratio <= 1.10
                print(f"[{mode}] W = {W:2d} {k:13s} {t[k]:8.1f} us ({b / t[k] / 1e6:5.2f} TB/s)  copy of equal bytes "
                      f"{cp:8.1f} us  ratio {ratio:.3f} {'ok' if ok else 'MISS'}  sgd_apply_multi "
                      f"{t['sgd_apply_multi']:8.1f} us ({t[k] / t['sgd_apply_multi']:.3f} x)", flush=True)
                if not ok:
                    misses.append((W, k, mode, round(ratio, 3)))
        del wires, fns
    print(f"cells above 1.10 x the copy of equal bytes: {misses if misses else 'none'}", flush=True)


if __name__ == "__main__":
    main()
