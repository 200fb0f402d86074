"""Robust-aggregation kernel timing (csrc/kernels/robust.hip) against the wire sum it replaces.

  python bench/robust_bench.py [--model resnet18] [--rank-workers 3,7,15,31] [--krum-workers 7,31]
                               [--groups 20] [--per-group 10]

On the model's trainable size, W fp16 wires: the device time of the rank kernel (trimmed T = 1 and
median; one launch) and of the multi-Krum trio (Gram + select + selected sum, F = 1), in one process,
the kernels taking turns, cache-warm and after a cache scrub (bench/q8_bench.py for the two
schemes). Yardsticks, timed beside them:
  sgd_apply_multi with the same W (no momentum, no image): its wire sum reads the same 2 W bytes per
    element, plus 4 read and 4 written for the parameters;
  a streaming fp32 copy moving the same number of bytes: 2 W + 4 per element for the rank kernel
    (W wires read, the estimate written), 4 W + 4 for krum (the wires are read twice).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--rank-workers", default="3,7,15,31")
    ap.add_argument("--krum-workers", default="7,31")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda"
    n = ParamLayout.from_module(build_model(a.model, 100)).param_numel
    rank_w = [int(w) for w in a.rank_workers.split(",")]
    krum_w = [int(w) for w in a.krum_workers.split(",")]
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    print(f"{a.model}: n = {n}", flush=True)
    agg, p = torch.zeros(n, device=dev), torch.randn(n, device=dev) * 0.05
    krum = K.KrumState(n, dev)
    misses = []
    for W in sorted(set(rank_w + krum_w)):
        wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
        fns, nbytes = {"sgd_apply_multi": lambda: K.sgd_apply_multi(p, wires, 1e-6, gscale=1.0 / W, n=n)}, {}

        def copy_of(b):
            src, dst = torch.zeros(b // 8, device=dev), torch.zeros(b // 8, device=dev)
            return lambda: dst.copy_(src)

        if W in rank_w:
            nbytes["trimmed"] = nbytes["median"] = n * (2 * W + 4)
            fns["trimmed"] = lambda: K.robust_rank(wires, agg, "trimmed", trim=1, c=float(W), n=n)
            fns["median"] = lambda: K.robust_rank(wires, agg, "median", c=float(W), n=n)
            fns["copy (rank bytes)"] = copy_of(n * (2 * W + 4))
        if W in krum_w:
            nbytes["krum"] = n * (4 * W + 4)

            def trio():
                K.robust_gram(wires, krum)
                K.robust_krum_select(krum, W, 1)
                K.robust_select_sum(wires, krum, agg, W - 1, c=float(W))

            fns["krum"] = trio
            fns["copy (krum bytes)"] = copy_of(n * (4 * W + 4))
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            t = time_alternating(fns, a.groups, a.per_group, scrub)
            for k, b in nbytes.items():
                cp = t["copy (krum bytes)" if k == "krum" else "copy (rank bytes)"]
                ratio = t[k] / cp
                ok = ratio <= 1.10
                print(f"[{mode}] W = {W:2d} {k:8s} {t[k]:8.1f} us ({b / t[k] / 1e6:5.2f} TB/s)  copy of equal bytes "
                      f"{cp:8.1f} us  ratio {ratio:.3f} {'ok' if ok else 'MISS'}  sgd_apply_multi "
                      f"{t['sgd_apply_multi']:8.1f} us ({t[k] / t['sgd_apply_multi']:.3f} x)", flush=True)
                if not ok:
                    misses.append((W, k, mode, round(ratio, 3)))
        del wires, fns
    print(f"cells above 1.10 x the copy of equal bytes: {misses if misses else 'none'}", flush=True)


if __name__ == "__main__":
    main()
