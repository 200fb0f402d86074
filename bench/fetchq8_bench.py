"""Timing of the delta fetch wire (--fetch-codec q8delta, parallel/fetchq8.py).

  python bench/fetchq8_bench.py [--models resnet18,resnet50] [--groups 20] [--per-group 10]
                                [--loopback fp32,q8delta] [--steps 50,250] [--only kernels|loopback]

Kernels, at every model's arena size, each pair taking turns in the same process (the timing
method, warm and cold, is bench/q8_bench.py's):

  * the server's encode (fetchq8_encode) against q8_encode from fp32 gradients: both move 13
    bytes per element, so the second is the yardstick;
  * the worker's add (q8_decode, add) against a streaming fp32 device copy of the same 9 bytes
    per element.

Loopback: run_local, ResNet-18, fp32, one worker, per fetch codec: milliseconds per step as the
difference of two runs of different length (setup and the graph capture cancel).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.utils.config import PSConfig  # noqa: E402


def arena_numel(model: str) -> int:
    from psx.parallel.runner import build_state

    return build_state(PSConfig(model=model).validate())[1].arena_numel


def kernels(models, groups, per_group):
    from bench.q8_bench import report, time_alternating
    from psx.ops import kernels as K
    from psx.parallel import fetchq8 as F
    from psx.parallel import q8 as Q

    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    blk = 1 + 4 / Q.BLOCK  # payload bytes per element (int8 + the block's scale share)
    for model in models:
        n = arena_numel(model)
        arena = torch.randn(n, device=dev) * 0.05
        shadow = arena + torch.randn(n, device=dev) * 1e-3
        payload = Q.empty_payload(n, dev)
        g32 = torch.randn(n, device=dev) * 1e-3
        enc = Q.Q8Codec(n, dev)
        local = shadow.clone()
        m = -(-9 * n // 8)  # fp32 elements whose copy moves 9 n bytes
        src, dst = torch.randn(m, device=dev), torch.empty(m, device=dev)
        print(f"{model}: arena {n} elements, fp32 fetch {4 * n / 1e6:.2f} MB, q8delta payload "
              f"{F.payload_bytes(n) / 1e6:.2f} MB", flush=True)
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            print(f"[{mode}] server encode", flush=True)
            t = time_alternating({"fetch": lambda: K.fetchq8_encode(arena, shadow, payload, n),
                                  "q8": lambda: K.q8_encode(g32, enc.resid, enc.payload, n)}, groups, per_group, scrub)
            report("fetchq8_encode", t["fetch"], n * (12 + blk))
            report("q8_encode, fp32 g (yardstick)", t["q8"], n * (12 + blk))
            print(f"  fetchq8_encode / q8_encode time: {t['fetch'] / t['q8']:.3f}  (expected <= 1.10)", flush=True)
            print(f"[{mode}] worker add", flush=True)
            t = time_alternating({"add": lambda: K.q8_decode(payload, local, n, 1.0, True),
                                  "copy": lambda: dst.copy_(src)}, groups, per_group, scrub)
            report("q8_decode, add", t["add"], n * (8 + blk))
            report("fp32 device copy (yardstick)", t["copy"], 8 * m)
            print(f"  q8_decode add / copy time: {t['add'] / t['copy']:.3f}", flush=True)
        del arena, shadow, payload, g32, enc, local, src, dst


def loopback(codecs, steps):
    from psx.parallel.runner import run_local

    lo, hi = steps
    for fc in codecs:
        secs = {}
        for s in (lo, hi):
            cfg = PSConfig(model="resnet18", batch_size=128, epochs=1, train_samples=128 * hi, eval_every=0, verbose=0,
                           mode="sync", workers=1, dtype="fp32", max_steps=s, fetch_codec=fc).validate()
            res = run_local(cfg, log=lambda *a, **k: None)
            secs[s] = sum(res["workers"][0]["epoch_times_seconds"])
            fetched = res["server"]["bytes_fetched"] / s
        ms = (secs[hi] - secs[lo]) / (hi - lo) * 1e3
        print(f"loopback resnet18 fp32 batch 128, --fetch-codec {fc}: {ms:.3f} ms/step "
              f"({lo} steps {secs[lo]:.2f} s, {hi} steps {secs[hi]:.2f} s; {fetched / 1e6:.2f} MB fetched per round)",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--loopback", default="fp32,q8delta")
    ap.add_argument("--steps", default="50,250")
    ap.add_argument("--only", choices=["kernels", "loopback"], default=None)
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if a.only != "loopback":
        kernels(a.models.split(","), a.groups, a.per_group)
    if a.only != "kernels":
        loopback([c for c in a.loopback.split(",") if c], tuple(int(s) for s in a.steps.split(",")))


if __name__ == "__main__":
    main()
