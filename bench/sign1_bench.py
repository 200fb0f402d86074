"""sign1 codec kernel timing (csrc/kernels/sign1.hip) next to the q8 and fp16-wire kernels.

  python bench/sign1_bench.py [--models resnet18,resnet50] [--workers 1,7] [--groups 20] [--per-group 10]
  python bench/sign1_bench.py --step-time [--steps 200] [--warmup 30]

Encode (fp32 and fp16 gradient input) next to q8_encode, and the server update from W payloads
(sign1_apply_multi) next to q8_apply_multi on W q8 payloads and sgd_apply_multi on W fp16 wires:
plain and momentum 0.9 + weight decay, bf16 image on and off, warm and cold (bench/q8_bench.py
explains both), all kernels of a comparison taking turns in one process, medians. Each figure
comes with the bytes the kernel must move, computed from n and W, and the resulting rate.

The yardstick: time relative to the compared kernel at most the ratio of the bytes moved x 1.10;
a line that misses it ends in MISS.

--step-time: ms per step of the one-GPU W = 1 sync loopback (fetch + step + push + server update)
with --codec fp16, q8 and sign1, alternating, two rounds.
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
from psx.parallel import q8 as Q  # noqa: E402
from psx.parallel import sign1 as S  # noqa: E402

SLACK = 1.10
B_S1 = 4 / S.BLOCK + 1 / 8   # payload bytes per parameter: the block's scale share + one bit
B_Q8 = 4 / Q.BLOCK + 1       # the block's scale share + one int8


def report(name: str, us: float, nbytes: float):
    print(f"  {name:40s} {us:8.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / us / 1e6:6.2f} TB/s", flush=True)


def yardstick(what: str, us: float, nbytes: float, ref: str, ref_us: float, ref_bytes: float):
    t, b = us / ref_us, nbytes / ref_bytes
    print(f"    {what} / {ref}: time {t:.3f}, bytes {b:.3f}, allowed {b * SLACK:.3f}"
          f"{'  MISS' if t > b * SLACK else ''}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--step-time", action="store_true", help="only the one-GPU loopback step time per codec")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.step_time:
        t = {}
        for rep in range(2):  # alternating, two rounds
            for codec in ("fp16", "q8", "sign1"):
                t.setdefault(codec, []).append(step_time("sgd", a.steps, a.warmup, codec=codec))
        for codec, v in t.items():
            print(f"step time, --codec {codec}: " + ", ".join(f"{x:.3f}" for x in v) + " ms/step", flush=True)
        return
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    modes = (("warm", None), ("cold", scratch.zero_))
    for model in a.models.split(","):
        n = ParamLayout.from_module(build_model(model, 100)).param_numel
        print(f"{model}: n = {n}: sign1 payload {S.payload_bytes(n) / 1e6:.2f} MB, q8 payload "
              f"{Q.payload_bytes(n) / 1e6:.2f} MB, fp16 wire {2 * n / 1e6:.2f} MB", flush=True)
        g32 = torch.randn(n, device=dev) * 1e-3
        g16 = g32.half()
        es, eq = S.Sign1Codec(n, dev), Q.Q8Codec(n, dev)
        fns = {"s32": lambda: es.encode(g32), "s16": lambda: es.encode(g16), "q32": lambda: eq.encode(g32),
               "q16": lambda: eq.encode(g16)}
        for mode, scrub in modes:
            print(f"[{mode}] encode", flush=True)
            t = time_alternating(fns, a.groups, a.per_group, scrub)
            for gb, tag in ((4, "32"), (2, "16")):  # g, resid read, resid written, the payload
                bs, bq = n * (gb + 8 + B_S1), n * (gb + 8 + B_Q8)
                report(f"sign1_encode, fp{tag} g", t["s" + tag], bs)
                report(f"q8_encode, fp{tag} g", t["q" + tag], bq)
                yardstick("sign1", t["s" + tag], bs, "q8", t["q" + tag], bq)
        for W in [int(w) for w in a.workers.split(",")]:
            ps, pq, pf = (torch.randn(n, device=dev) for _ in range(3))
            bufs = [torch.zeros(n, device=dev) for _ in range(3)]
            img = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            wires = [(torch.randn(n, device=dev) * 1e-3).half() for _ in range(W)]
            pays_s, pays_q = [], []
            for w in wires:
                es.resid.zero_()
                eq.resid.zero_()
                pays_s.append(es.encode(w).clone())
                pays_q.append(eq.encode(w).clone())
            for mom in (False, True):
                for img_on in (False, True):
                    im = img if img_on else None
                    hp = dict(gscale=1.0 / W, n=n, img=im)
                    if mom:
                        hp.update(momentum=0.9, wd=5e-4)
                    kb = [dict(hp, buf=b) if mom else hp for b in bufs]
                    fns = {"sign1": lambda: K.sign1_apply_multi(ps, pays_s, 1e-6, **kb[0]),
                           "q8": lambda: K.q8_apply_multi(pq, pays_q, 1e-6, **kb[1]),
                           "fp16": lambda: K.sgd_apply_multi(pf, wires, 1e-6, **kb[2])}
                    state = 8 + 8 * mom + 2 * img_on  # p [and buf] read and written [, the image written]
                    nb = {"sign1": n * (state + W * B_S1), "q8": n * (state + W * B_Q8), "fp16": n * (state + 2 * W)}
                    for mode, scrub in modes:
                        print(f"[{mode}] server update, W = {W}, {'momentum 0.9 + wd' if mom else 'plain'}, image "
                              f"{'on' if img_on else 'off'}", flush=True)
                        t = time_alternating(fns, a.groups, a.per_group, scrub)
                        report("sign1_apply_multi (sign1 payloads)", t["sign1"], nb["sign1"])
                        report("q8_apply_multi (q8 payloads)", t["q8"], nb["q8"])
                        report("sgd_apply_multi (fp16 wires)", t["fp16"], nb["fp16"])
                        for ref in ("q8", "fp16"):
                            yardstick("sign1", t["sign1"], nb["sign1"], ref, t[ref], nb[ref])


if __name__ == "__main__":
    main()
