"""LAMB update timing (csrc/kernels/lamb.hip) against the AdamW update, the LARS pair and a copy.

  python bench/lamb_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 20] [--per-group 10]

On the real layouts of the models (the segment table of every trainable tensor), W fp16 wires, bf16
image off and on: the device time of the two LAMB launches (lamb_moments + lamb_apply) next to the
one adamw_apply_multi launch, the two LARS launches (momentum 0.9) and a streaming fp32 copy that
moves the LAMB pair's byte count, all in one process, taking turns (bench/q8_bench.py
time_alternating: cache-warm, and after a cache scrub). Bytes per element:
  lamb pair         : 2 W + 12 read (wires, p, m, v), 12 written (u, m, v); 8 read (u, p), 4 written (p)
                      = 2 W + 36                                                  [+ 2 with the image]
  adamw_apply_multi : 2 W + 12 read, 12 written = 2 W + 24                        [+ 2 with the image]
  lars pair         : 2 W + 4 read, 4 written; 12 read, 8 written = 2 W + 28      [+ 2 with the image]
The yardstick is bytes: the LAMB pair may take (2 W + 36 [+ 2]) / (2 W + 24 [+ 2]) of AdamW's time
in the same cell, times the 1.10 allowed for one extra launch boundary; a cell above it is marked
"MISS".

--step-time: the one-GPU step time (device time per step of a W = 1 sync loopback, ResNet-18,
batch 128, fp32 engine) with --optimizer lamb (lr 2e-3, weight decay 1e-2) against the SGD server
(momentum 0.9, weight decay 5e-4).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import psx  # noqa: E402,F401
from bench.lars_bench import step_time  # noqa: E402
from bench.q8_bench import time_alternating  # noqa: E402
from psx.models.layout import ParamLayout  # noqa: E402
from psx.models.resnet import build_model  # noqa: E402
from psx.ops import kernels as K  # noqa: E402

MARGIN = 1.10


def report(name: str, us: float, nbytes: float, copy_us: float, copy_bytes: float):
    tbs, ctbs = nbytes / us / 1e6, copy_bytes / copy_us / 1e6
    print(f"  {name:42s} {us:8.1f} us  {nbytes / 1e6:8.1f} MB  {tbs:6.2f} TB/s  {tbs / ctbs:5.2f} of copy", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time, lamb vs sgd")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        runs = {"sgd": dict(), "lamb": dict(lr=2e-3, momentum=0.0, weight_decay=1e-2)}
        t = {}
        for rep in range(2):  # alternating, two rounds
            for opt, hp in runs.items():
                t.setdefault(opt, []).append(step_time(opt, a.steps, a.warmup, **hp))
        for opt, v in t.items():
            print(f"step time, --optimizer {opt}: " + ", ".join(f"{x:.3f}" for x in v) + " ms/step", flush=True)
        return
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    misses = cells = 0
    for model in a.models.split(","):
        lay = ParamLayout.from_module(build_model(model, 100))
        n = lay.param_numel
        tab, tab2 = K.lars_table(lay, dev), K.lars_table(lay, dev)
        print(f"{model}: n = {n}, {tab.ntensors} tensors, {tab.nblocks} workgroups of {K.LARS_CHUNK}", flush=True)
        for W in [int(w) for w in a.workers.split(",")]:
            p, p2, p3 = (torch.randn(n, device=dev) * 0.05 for _ in range(3))
            m, v, m2, v2, buf = (torch.zeros(n, device=dev) for _ in range(5))
            stage, stage2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            img = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            for img_on in (False, True):
                im = img if img_on else None
                bl, ba, br = (n * (2 * W + k + 2 * img_on) for k in (36, 24, 28))
                cl = torch.randn(bl // 8, device=dev)
                dl = torch.empty_like(cl)
                fns = {"lamb": lambda: K.lamb_apply_multi(p, wires, stage, m, v, tab, 1e-6, 1000, gscale=1.0 / W,
                                                          wd=1e-2, n=n, img=im),
                       "adamw": lambda: K.adamw_apply_multi(p2, wires, m2, v2, 1e-6, 1000, gscale=1.0 / W, wd=1e-2,
                                                            n=n, img=im),
                       "lars": lambda: K.lars_apply_multi(p3, wires, stage2, tab2, 1e-6, gscale=1.0 / W, momentum=0.9,
                                                          wd=5e-4, buf=buf, n=n, img=im),
                       "copy": lambda: dl.copy_(cl)}
                for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                    print(f"[{mode}] server update, W = {W}, image {'on' if img_on else 'off'}", flush=True)
                    t = time_alternating(fns, a.groups, a.per_group, scrub)
                    report("lamb pair (moments + apply, fp16 wires)", t["lamb"], bl, t["copy"], bl)
                    report("adamw_apply_multi (fp16 wires)", t["adamw"], ba, t["copy"], bl)
                    report("lars pair, momentum (fp16 wires)", t["lars"], br, t["copy"], bl)
                    ratio, bound = t["lamb"] / t["adamw"], bl / ba * MARGIN
                    miss = ratio > bound
                    misses, cells = misses + miss, cells + 1
                    print(f"  lamb / adamw time: {ratio:.3f}  (bytes {bl / ba:.3f}, bound {bound:.3f})"
                          f"{'  MISS' if miss else ''}   lamb / lars time: {t['lamb'] / t['lars']:.3f}", flush=True)
        r = tab.ratios[torch.tensor(tab.adapt, device=dev)]
        print(f"  ratios of the last update: min {float(r.min()):.3e} median {float(r.median()):.3e} "
              f"max {float(r.max()):.3e}", flush=True)
    print(f"{misses} of {cells} cells miss the byte yardstick", flush=True)


if __name__ == "__main__":
    main()
