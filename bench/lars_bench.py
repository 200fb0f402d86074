"""LARS update timing (csrc/kernels/lars.hip) against the momentum SGD update it replaces.

  python bench/lars_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 20] [--per-group 10]

On the real layouts of the models (the segment table of every trainable tensor), W fp16 wires:
the device time of the two LARS launches (lars_norms + lars_apply, momentum 0.9, weight decay
5e-4, bf16 image off) next to sgd_apply_multi with the same momentum and weight decay, in the same
process, the two alternating. Each figure comes with the bytes the kernels must move per element
  lars_norms: 2 W + 4 read (wires, w), 4 written (the staged sum)
  lars_apply: 12 read (staged sum, w, v), 8 written (w, v)        [+ 2 with the image]
  sgd_apply_multi: 2 W + 8 read, 8 written
the resulting rate, and that rate as a fraction of a streaming fp32 copy of the same size measured
here the same way (warm and cold, see bench/q8_bench.py for the two schemes). The dense entry
(norms from an already summed staging buffer) is timed at W = 1.

--step-time: the one-GPU step time (device time per step of a W = 1 sync loopback, ResNet-18,
batch 128, fp32 engine) with --optimizer lars against the SGD server, both with momentum 0.9 and
weight decay 5e-4.
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


def report(name: str, us: float, nbytes: float, copy_tbs: float):
    tbs = nbytes / us / 1e6
    print(f"  {name:40s} {us:8.1f} us  {nbytes / 1e6:8.1f} MB  {tbs:6.2f} TB/s  {tbs / copy_tbs:5.2f} of copy",
          flush=True)


def step_time(optimizer: str, steps: int, warmup: int, batch: int = 128, **hparams) -> float:
    """ms per step of a W = 1 sync loopback (fetch + step + push + server update). ``hparams``
    override the server's lr / momentum / weight_decay (bench/adamw_bench.py)."""
    from psx.parallel.compute import make_compute
    from psx.parallel.runner import _wire_dtype, build_state, make_local_channel
    from psx.parallel.server import ParameterServer
    from psx.parallel.worker import Worker
    from psx.utils.config import PSConfig
    from psx.utils.data import DeviceDataset

    dev = torch.device("cuda", 0)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    hp.update(hparams)
    cfg = PSConfig(model="resnet18", mode="sync", workers=1, batch_size=batch, epochs=10 ** 6,
                   train_samples=10000, eval_every=0, verbose=0, optimizer=optimizer, **hp).validate()
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
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time, lars vs sgd")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        t = {}
        for rep in range(2):  # alternating, two rounds
            for opt in ("sgd", "lars"):
                t.setdefault(opt, []).append(step_time(opt, a.steps, a.warmup))
        for opt, v in t.items():
            print(f"step time, --optimizer {opt} --momentum 0.9 --weight-decay 5e-4: "
                  + ", ".join(f"{x:.3f}" for x in v) + " ms/step", flush=True)
        return
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    hp = dict(momentum=0.9, wd=5e-4)
    for model in a.models.split(","):
        lay = ParamLayout.from_module(build_model(model, 100))
        n = lay.param_numel
        tab = K.lars_table(lay, dev)
        print(f"{model}: n = {n}, {tab.ntensors} tensors, {tab.nblocks} workgroups of {K.LARS_CHUNK}", flush=True)
        src, dst = torch.randn(n, device=dev), torch.empty(n, device=dev)
        copy = {}
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            us = time_alternating({"copy": lambda: dst.copy_(src)}, a.groups, a.per_group, scrub)["copy"]
            copy[mode] = 8 * n / us / 1e6
            print(f"[{mode}] streaming fp32 copy: {us:.1f} us, {copy[mode]:.2f} TB/s", flush=True)
        for W in [int(w) for w in a.workers.split(",")]:
            p = torch.randn(n, device=dev) * 0.05
            p2 = p.clone()
            v, v2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            stage = torch.zeros(n, device=dev)
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            fns = {"lars": lambda: K.lars_apply_multi(p, wires, stage, tab, 1e-6, gscale=1.0 / W, buf=v, **hp),
                   "sgd": lambda: K.sgd_apply_multi(p2, wires, 1e-6, gscale=1.0 / W, buf=v2, n=n, **hp)}
            if W == 1:
                fns["lars_dense"] = lambda: K.lars_apply(p, stage, tab, 1e-6, gscale=1.0, buf=v, **hp)
            for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                print(f"[{mode}] server update, W = {W}", flush=True)
                t = time_alternating(fns, a.groups, a.per_group, scrub)
                report("lars pair (norms + apply, fp16 wires)", t["lars"], n * (2 * W + 8 + 20), copy[mode])
                if "lars_dense" in t:
                    report("lars pair, dense entry", t["lars_dense"], n * (8 + 20), copy[mode])
                report("sgd_apply_multi, momentum (fp16 wires)", t["sgd"], n * (2 * W + 16), copy[mode])
                print(f"  lars / sgd time: {t['lars'] / t['sgd']:.3f}", flush=True)
        r = tab.ratios[torch.tensor(tab.adapt, device=dev)]
        print(f"  trust ratios of the last update: min {float(r.min()):.3e} median {float(r.median()):.3e} "
              f"max {float(r.max()):.3e}", flush=True)


if __name__ == "__main__":
    main()
