"""Muon update timing (csrc/kernels/muon.hip) next to the LAMB pair.

  python bench/muon_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 10] [--per-group 5]
                             [--peak-tflops X]

On the real layouts of the models, W fp16 wires, momentum 0.95, five Newton-Schulz steps: the
device time of the 1 + 3 * 5 + 1 launches of muon_apply_multi and of the two LAMB launches, in one
process, taking turns (bench/q8_bench.py time_alternating: cache-warm, and after a cache scrub).
The update is the chain: its multiply-adds (MuonTable.flops: 4 m^2 n + 2 m^3 per matrix and step,
symmetric halves and pads not discounted) over the whole update's time is the achieved TFLOP/s
printed, a lower bound on the chain's own; --peak-tflops (the fp32 number bench/micro/mfma_peak.hip
prints on the same box) adds the share of the fp32 matrix peak. Nothing is asserted.

--step-time: the one-GPU step time (W = 1 sync loopback, ResNet-18, batch 128, fp32 engine) with
--optimizer muon (lr 0.02, momentum 0.95, weight decay 0.01) against the SGD server.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--per-group", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=0.0, help="fp32 MFMA peak of this box (mfma_peak.hip)")
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time, muon vs sgd")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        runs = {"sgd": dict(), "muon": dict(lr=0.02, momentum=0.95, weight_decay=0.01)}
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
        lay = ParamLayout.from_module(build_model(model, 100))
        n = lay.param_numel
        tab, tab2 = K.lars_table(lay, dev), K.lars_table(lay, dev)
        mtab = K.MuonTable(lay, dev, tab)
        gf = mtab.flops(5) / 1e9
        ws = sum(t.numel() for t in mtab.x + [mtab.a, mtab.b]) * 4 / 2 ** 20
        print(f"{model}: n = {n}, {mtab.nmat} matrices of {tab.ntensors} tensors, chain {gf:.1f} GFLOP per update, "
              f"tiles {[int(m.shape[0]) for m in mtab.maps]} (SyrkA, SyrkB, NN), workspaces {ws:.0f} MiB", flush=True)
        for W in [int(w) for w in a.workers.split(",")]:
            p, p2 = (torch.randn(n, device=dev) * 0.05 for _ in range(2))
            buf, m, v, stage, stage2 = (torch.zeros(n, device=dev) for _ in range(5))
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            fns = {"muon": lambda: K.muon_apply_multi(p, wires, stage, buf, tab, mtab, 1e-6, gscale=1.0 / W,
                                                      momentum=0.95, wd=1e-2, n=n),
                   "lamb": lambda: K.lamb_apply_multi(p2, wires, stage2, m, v, tab2, 1e-6, 1000, gscale=1.0 / W,
                                                      wd=1e-2, n=n)}
            for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                t = time_alternating(fns, a.groups, a.per_group, scrub)
                tf = gf / t["muon"] * 1e3  # GFLOP per us = 1000 TFLOP/s
                share = f", {100 * tf / a.peak_tflops:.1f}% of the fp32 MFMA peak" if a.peak_tflops else ""
                print(f"[{mode}] W = {W}: muon update {t['muon']:9.1f} us ({tf:.1f} TFLOP/s{share}), lamb pair "
                      f"{t['lamb']:7.1f} us", flush=True)
        r = tab.ratios[torch.tensor(tab.adapt, device=dev)]
        print(f"  |U|_F of the last update: min {float(r.min()):.3e} median {float(r.median()):.3e} "
              f"max {float(r.max()):.3e}", flush=True)


if __name__ == "__main__":
    main()
