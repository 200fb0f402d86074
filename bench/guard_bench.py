"""Gradient-guard update timing (csrc/kernels/gguard.hip) against the SGD update it wraps.

  python bench/guard_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 20] [--per-group 10]

On the models' trainable sizes, W fp16 wires, bf16 image on: the device time of the three guard
launches (guard_norms + guard_finish + guard_apply, --clip-norm far above the norm so that the
round is applied unscaled) next to sgd_apply_multi with the same momentum and weight decay, in the
same process, the two alternating, cache-warm and after a cache scrub (bench/q8_bench.py for the
two schemes). Two optimizer settings: plain (no momentum, no weight decay) and momentum 0.9 with
weight decay 5e-4. Bytes the kernels must move per element:
  guard_norms    : 2 W read, 4 written (the staged sum)
  guard_apply    : 8 read (staged sum, w), 4 written, + 2 with the image, + 8 with momentum
  sgd_apply_multi: 2 W + 4 read, 4 written, + 2, + 8
so the expected time ratio is (2 W + 18) / (2 W + 10) without and (2 W + 26) / (2 W + 18) with
momentum; a cell whose measured ratio exceeds that by more than 10 % (launch gaps, the small middle
launch) is marked MISS. A skipped round (one inf in a wire: guard_apply returns at once) is timed
beside them; expect it near the norms pass alone.

--step-time: the one-GPU step time (device time per step of a W = 1 sync loopback, ResNet-18,
batch 128, fp32 engine) with --clip-norm 1e9 / --skip-nonfinite against the unguarded server.
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


def step_time(guard: dict, steps: int, warmup: int, batch: int = 128) -> float:
    """ms per step of a W = 1 sync loopback (fetch + step + push + server update)."""
    from psx.parallel.compute import make_compute
    from psx.parallel.runner import _wire_dtype, build_state, make_local_channel
    from psx.parallel.server import ParameterServer
    from psx.parallel.worker import Worker
    from psx.utils.config import PSConfig
    from psx.utils.data import DeviceDataset

    dev = torch.device("cuda", 0)
    cfg = PSConfig(model="resnet18", mode="sync", workers=1, lr=0.05, batch_size=batch, epochs=10 ** 6,
                   train_samples=10000, eval_every=0, verbose=0, **guard).validate()
    quiet = lambda *a, **k: None  # noqa: E731
    model, lay, arena, counters = build_state(cfg)
    srv = ParameterServer(cfg, lay, arena.clone(), counters, device=dev, total_workers=1, log=quiet)
    comp = make_compute(model, lay, batch, dev, "resnet18", _wire_dtype(cfg), seed=0, use_graph=True, dtype="fp32")
    train = DeviceDataset.synthetic_hard(10000, device=dev)
    wk = Worker(cfg, comp, make_local_channel(cfg, srv, lay, dev), train, None, worker_name="w0", rank=0, log=quiet,
                requested_id=0)
    wk.connect_to_server()
    wk.setup_data()
    batches = wk.sampler.epoch_indices(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + steps):
        if i == warmup:
            a.record()
        wk.fetch_parameters()
        wk.train_local_batch(batches[i % len(batches)])
        wk.window_push(i % len(batches), len(batches), 1)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time, guard on vs off")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        cfgs = {"off": {}, "--skip-nonfinite": dict(skip_nonfinite=True), "--clip-norm 1e9": dict(clip_norm=1e9)}
        t = {}
        for rep in range(2):  # alternating, two rounds
            for name, g in cfgs.items():
                t.setdefault(name, []).append(step_time(g, a.steps, a.warmup))
        for name, v in t.items():
            print(f"step time, guard {name}: " + ", ".join(f"{x:.3f}" for x in v) + " ms/step", flush=True)
        return
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    misses = []
    for model in a.models.split(","):
        n = ParamLayout.from_module(build_model(model, 100)).param_numel
        st, st_bad = K.GuardState(n, dev), K.GuardState(n, dev)
        print(f"{model}: n = {n}, {st.nblocks} workgroups of {K.GUARD_CHUNK}", flush=True)
        for W in [int(w) for w in a.workers.split(",")]:
            p = torch.randn(n, device=dev) * 0.05
            p2, p3 = p.clone(), p.clone()
            v, v2, v3 = (torch.zeros(n, device=dev) for _ in range(3))
            img, img2, img3 = (torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(3))
            stage, stage_bad = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            bad = [wires[0].clone()] + wires[1:]
            bad[0][n // 2] = float("inf")
            for mom, hp in (("plain", dict(momentum=0.0, wd=0.0)), ("momentum 0.9, wd 5e-4", dict(momentum=0.9, wd=5e-4))):
                m = bool(hp["momentum"])
                fns = {"guard": lambda: K.guard_apply_multi(p, wires, stage, st, 1e-6, gscale=1.0 / W, clip_norm=1e30,
                                                            buf=v if m else None, img=img, **hp),
                       "skipped": lambda: K.guard_apply_multi(p3, bad, stage_bad, st_bad, 1e-6, gscale=1.0 / W,
                                                              clip_norm=1e30, buf=v3 if m else None, img=img3, **hp),
                       "sgd": lambda: K.sgd_apply_multi(p2, wires, 1e-6, gscale=1.0 / W, buf=v2 if m else None, n=n,
                                                        img=img2, **hp)}
                want = (2 * W + 26) / (2 * W + 18) if m else (2 * W + 18) / (2 * W + 10)
                for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                    t = time_alternating(fns, a.groups, a.per_group, scrub)
                    ratio = t["guard"] / t["sgd"]
                    ok = ratio <= want * 1.10
                    gb = n * (2 * W + (26 if m else 18))
                    print(f"[{mode}] {model} W = {W}, {mom}: guard {t['guard']:7.1f} us ({gb / t['guard'] / 1e6:5.2f} "
                          f"TB/s)  sgd_apply_multi {t['sgd']:7.1f} us  skipped round {t['skipped']:7.1f} us  "
                          f"guard / sgd {ratio:.3f} (bytes {want:.3f}, x 1.10 = {want * 1.10:.3f}) "
                          f"{'ok' if ok else 'MISS'}", flush=True)
                    if not ok:
                        misses.append((model, W, mom, mode, round(ratio, 3), round(want * 1.10, 3)))
        r, rb = st.read(), st_bad.read()
        assert r["skipped_rounds"] == 0 and r["clipped_rounds"] == 0 and rb["skipped_rounds"] == rb["rounds"] > 0
    print(f"cells above bytes ratio x 1.10: {misses if misses else 'none'}", flush=True)


if __name__ == "__main__":
    main()
