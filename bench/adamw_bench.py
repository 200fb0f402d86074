"""AdamW update timing (csrc/kernels/adamw.hip) against the momentum SGD update and a copy.

  python bench/adamw_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 20] [--per-group 10]

On the real layouts of the models, W fp16 wires, bf16 image off and on: the device time of the one
AdamW launch next to sgd_apply_multi (momentum 0.9, weight decay 5e-4) and next to streaming fp32
copies that move the same number of bytes as each of the two, all in one process, taking turns
(bench/q8_bench.py time_alternating: cache-warm, and after a cache scrub). Bytes per element:
  adamw_apply_multi: 2 W + 12 read (wires, p, m, v), 12 written (p, m, v)   [+ 2 with the image]
  sgd_apply_multi  : 2 W + 8 read (wires, p, buf), 8 written (p, buf)       [+ 2 with the image]
Every figure is printed with its rate and that rate as a fraction of its copy's; a fraction below
0.75 is marked "MISS".

--step-time: the one-GPU step time (device time per step of a W = 1 sync loopback, ResNet-18,
batch 128, fp32 engine) with --optimizer adamw (lr 1e-3, weight decay 1e-2) against the SGD server
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

MISS = 0.75


def report(name: str, us: float, nbytes: float, copy_us: float):
    tbs, ctbs = nbytes / us / 1e6, nbytes / copy_us / 1e6
    frac = tbs / ctbs
    print(f"  {name:42s} {us:8.1f} us  {nbytes / 1e6:8.1f} MB  {tbs:6.2f} TB/s  copy {ctbs:5.2f} TB/s  "
          f"{frac:5.2f} of copy{'  MISS' if frac < MISS else ''}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time, adamw vs sgd")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        runs = {"sgd": dict(), "adamw": dict(lr=1e-3, momentum=0.0, weight_decay=1e-2)}
        t = {}
        for rep in range(2):  # alternating, two rounds
            for opt, hp in runs.items():
                t.setdefault(opt, []).append(step_time(opt, a.steps, a.warmup, **hp))
        for opt, v in t.items():
            print(f"step time, --optimizer {opt}: " + ", ".join(f"{x:.3f}" for x in v) + " ms/step", flush=True)
        return
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    for model in a.models.split(","):
        n = ParamLayout.from_module(build_model(model, 100)).param_numel
        print(f"{model}: n = {n}", flush=True)
        for W in [int(w) for w in a.workers.split(",")]:
            p = torch.randn(n, device=dev) * 0.05
            p2 = p.clone()
            m, v, buf = (torch.zeros(n, device=dev) for _ in range(3))
            img = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            for img_on in (False, True):
                im = img if img_on else None
                ba, bs = n * (2 * W + 24 + 2 * img_on), n * (2 * W + 16 + 2 * img_on)
                ca, cs = (torch.randn(b // 8, device=dev) for b in (ba, bs))
                da, ds = torch.empty_like(ca), torch.empty_like(cs)
                fns = {"adamw": lambda: K.adamw_apply_multi(p, wires, m, v, 1e-6, 1000, gscale=1.0 / W, wd=1e-2, n=n,
                                                            img=im),
                       "sgd": lambda: K.sgd_apply_multi(p2, wires, 1e-6, gscale=1.0 / W, momentum=0.9, wd=5e-4,
                                                        buf=buf, n=n, img=im),
                       "copy_a": lambda: da.copy_(ca), "copy_s": lambda: ds.copy_(cs)}
                for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                    print(f"[{mode}] server update, W = {W}, image {'on' if img_on else 'off'}", flush=True)
                    t = time_alternating(fns, a.groups, a.per_group, scrub)
                    report("adamw_apply_multi (fp16 wires)", t["adamw"], ba, t["copy_a"])
                    report("sgd_apply_multi, momentum (fp16 wires)", t["sgd"], bs, t["copy_s"])
                    print(f"  adamw / sgd time: {t['adamw'] / t['sgd']:.3f}", flush=True)


if __name__ == "__main__":
    main()
