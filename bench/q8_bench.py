"""q8 codec kernel timing (csrc/kernels/q8.hip) against the fp16-wire kernels they replace.

  python bench/q8_bench.py [--n 11220132] [--workers 1,7] [--groups 20] [--per-group 10]

Encode (fp32 and fp16 gradient input) and the server update from W payloads (q8_apply_multi)
next to sgd_apply_multi on W fp16 wires at the same n, in the same process, the two alternating.
Each figure comes with the bytes the kernel must move, computed from n and W, and the resulting
rate:

  * warm: device time of ``per-group`` back-to-back launches between two events, median over
    ``groups`` groups. Below ~256 MB of working set the operands stay in the Infinity Cache
    between launches, so this rate can exceed what HBM delivers;
  * cold: one launch between two events after a 512 MiB scrub of the cache (a training step
    runs between two updates of a real round), median over groups * per-group launches.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.ops import kernels as K  # noqa: E402
from psx.parallel import q8 as Q  # noqa: E402


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_alternating(fns: dict, groups: int, per_group: int, scrub=None) -> dict:
    """Median device microseconds per launch of every fn, the fns taking turns group by group
    (warm: per_group launches per event pair; cold: scrub, then one launch per event pair)."""
    for f in fns.values():  # warm-up: code objects loaded, buffers touched
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    pairs = {k: [] for k in fns}
    for _ in range(groups):
        for k, f in fns.items():
            if scrub is None:
                a, b = _events()
                a.record()
                for _ in range(per_group):
                    f()
                b.record()
                pairs[k].append((a, b, per_group))
            else:
                for _ in range(per_group):
                    scrub()
                    a, b = _events()
                    a.record()
                    f()
                    b.record()
                    pairs[k].append((a, b, 1))
    torch.cuda.synchronize()  # before any clock is read
    return {k: statistics.median(a.elapsed_time(b) * 1e3 / m for a, b, m in v) for k, v in pairs.items()}


def report(name: str, us: float, nbytes: float):
    print(f"  {name:34s} {us:8.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / us / 1e6:6.2f} TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_220_132)
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    a = ap.parse_args()
    n, dev = a.n, "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    blk = 1 + 4 / Q.BLOCK  # payload bytes per parameter (int8 + the block's scale share)
    g32 = torch.randn(n, device=dev) * 1e-3
    g16 = g32.half()
    enc = Q.Q8Codec(n, dev)
    print(f"n = {n}: q8 payload {Q.payload_bytes(n) / 1e6:.2f} MB, fp16 wire {2 * n / 1e6:.2f} MB", flush=True)
    for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
        print(f"[{mode}] encode", flush=True)
        t = time_alternating({"fp32": lambda: enc.encode(g32), "fp16": lambda: enc.encode(g16)}, a.groups,
                             a.per_group, scrub)
        report("q8_encode, fp32 g", t["fp32"], n * (12 + blk))
        report("q8_encode, fp16 g", t["fp16"], n * (10 + blk))
    for W in [int(w) for w in a.workers.split(",")]:
        p = torch.randn(n, device=dev)
        wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
        pays = []
        for w in wires:
            enc.resid.zero_()
            pays.append(enc.encode(w).clone())
        fns = {"q8": lambda: K.q8_apply_multi(p, pays, 1e-6, gscale=1.0 / W, n=n),
               "fp16": lambda: K.sgd_apply_multi(p, wires, 1e-6, gscale=1.0 / W, n=n)}
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            print(f"[{mode}] server update, W = {W}", flush=True)
            t = time_alternating(fns, a.groups, a.per_group, scrub)
            report("q8_apply_multi (q8 payloads)", t["q8"], n * (8 + W * blk))
            report("sgd_apply_multi (fp16 wires)", t["fp16"], n * (8 + 2 * W))
            print(f"  q8 / fp16 time: {t['q8'] / t['fp16']:.3f}", flush=True)


if __name__ == "__main__":
    main()
