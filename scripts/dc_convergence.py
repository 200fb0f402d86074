#!/usr/bin/env python3
"""Does delay compensation recover the async accuracy gap? A recorded comparison, not a test.

Four kinds of curve on one MI355X, all on the loopback (parallel/runner.py run_local), W workers,
ResNet-18, the ``hard`` synthetic set (20 % label noise), --bn-sync, evaluation by worker 0 after
every epoch:

* ``sync``            W-worker sync rounds (the averaged update): the accuracy to recover;
* ``async``           the loopback async path: pushes interleave round-robin, so every push has
                      staleness exactly W - 1 and the run is reproducible; --staleness-bound is set
                      high enough that nothing is rejected;
* ``async_dc_const``  the same with --dc-lambda L, one curve per L of --lambdas-const;
* ``async_dc_adapt``  the same with --dc-lambda L --dc-adaptive, one curve per L of --lambdas-adapt;
* ``async_guard``     the async run with --skip-nonfinite alone (the update unchanged): it measures
                      the mean global norm of the applied gradients, ``norm_mean``;
* ``async_clip``      the async run with --clip-norm C, one curve per fraction f of --clip-fractions,
                      C = f * norm_mean (does clipping the global norm steady the late epochs?).

Prints one line per curve (per-epoch test accuracy, final accuracy, compensated pushes, the
gradient guard's counters) and writes
``<out>/dc_convergence.json``.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psx  # noqa: E402,F401
from psx.parallel.runner import run_local  # noqa: E402
from psx.utils.config import PSConfig  # noqa: E402


def run(args, mode: str, **dc):
    cfg = PSConfig(model=args.model, mode=mode, workers=args.workers, lr=args.lr, batch_size=args.batch,
                   epochs=args.epochs, train_samples=args.train, test_samples=args.test, eval_every=1,
                   eval_workers="first", verbose=0, synthetic_kind="hard", bn_sync=True,
                   staleness_bound=8 * args.workers, **dc).validate()
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):  # METRICS_JSON lines of the loopback run
        res = run_local(cfg, log=lambda *a, **k: None)
    s, w0 = res["server"], res["workers"][0]
    return {"test_acc_per_epoch": w0["all_accuracies_percent"], "final_test_acc": w0["final_test_accuracy_percent"],
            "global_steps": s["global_steps_completed"], "rejected_pushes": s.get("rejected_pushes", 0),
            "average_staleness": s.get("average_gradient_staleness"),
            "delay_compensation": s.get("delay_compensation"), "gradient_guard": s.get("gradient_guard"),
            "seconds": round(time.time() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--train", type=int, default=20000)
    ap.add_argument("--test", type=int, default=2000)
    ap.add_argument("--lambdas-const", default="0.04,1.0")
    ap.add_argument("--lambdas-adapt", default="2.0")
    ap.add_argument("--clip-fractions", default="1,0.25",
                    help="--clip-norm curves at these fractions of the measured mean norm ('' = none)")
    ap.add_argument("--out", default="runs/dc_convergence")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    plan = [("sync", "sync", {}), ("async", "async", {})]
    plan += [(f"async_dc_const_{v}", "async", dict(dc_lambda=float(v))) for v in args.lambdas_const.split(",") if v]
    plan += [(f"async_dc_adapt_{v}", "async", dict(dc_lambda=float(v), dc_adaptive=True))
             for v in args.lambdas_adapt.split(",") if v]
    print(f"{args.model}, synthetic hard, W = {args.workers}, batch {args.batch}, lr {args.lr:g}, {args.epochs} epochs "
          f"of {args.train} samples, --bn-sync, fp32 engine, fp16 wire; test accuracy % of worker 0 per epoch",
          flush=True)
    fracs = [float(v) for v in args.clip_fractions.split(",") if v]
    if fracs:
        plan.append(("async_guard", "async", dict(skip_nonfinite=True)))
    runs = {}
    while plan:
        name, mode, dc = plan.pop(0)
        r = runs[name] = run(args, mode, **dc)
        comp, guard = r["delay_compensation"], r["gradient_guard"]
        if name == "async_guard":  # the clipping bounds come from this run's mean norm
            plan += [(f"async_clip_{f:g}xmean", "async", dict(clip_norm=f * guard["norm_mean"])) for f in fracs]
        print(f"{name:22s} acc/epoch {r['test_acc_per_epoch']} final {r['final_test_acc']:.2f}%  "
              f"updates {r['global_steps']} rejected {r['rejected_pushes']} mean staleness {r['average_staleness']}"
              + (f" compensated {comp['compensated_pushes']} uncompensated {comp['uncompensated_pushes']}"
                 if comp else "")
              + (f" clip_norm {guard['clip_norm']:.4g} clipped {guard['clipped_rounds']} skipped "
                 f"{guard['skipped_rounds']} norm mean {guard['norm_mean']:.4g} max {guard['norm_max']:.4g}"
                 if guard else "") + f"  ({r['seconds']} s)", flush=True)
    with open(os.path.join(args.out, "dc_convergence.json"), "w") as f:
        json.dump({"config": vars(args), "runs": runs}, f)


if __name__ == "__main__":
    main()
