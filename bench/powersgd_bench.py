"""PowerSGD codec kernel timing (csrc/kernels/powersgd.hip) next to the top-k encode and a streaming copy.

  python bench/powersgd_bench.py [--models resnet18,resnet50] [--ranks 4] [--workers 1,7] [--out FILE]

The device time of one encode (its four launches together: project, orth, backproject, residual;
fp32 and fp16 gradient input) and of psgd_decode from W payloads, warm and cold (bench/q8_bench.py
explains both), next to topk_encode and to a streaming fp32 copy that moves the same bytes, all
taking turns in one process, medians. The bytes an encode must move are about 24 per parameter
(g read; e read and M written; M read; M read, e written) and the decode's 4 (the sum written; the
factors are 0.05 per parameter and worker); each time is also given as a ratio of the copy's time
for those bytes. The table goes to stdout and to --out. No threshold is asserted.
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
from psx.parallel import powersgd as PS  # noqa: E402
from psx.parallel import topk as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--ranks", default="4")
    ap.add_argument("--workers", default="1,7")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "powersgd_kernels.txt"))
    a = ap.parse_args()
    dev = "cuda"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"bench/powersgd_bench.py on {torch.cuda.get_device_name(0)}: median device us over {a.groups} groups "
        f"(warm: {a.per_group} launches per event pair; cold: a 512 MiB scrub before every launch)")
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    modes = (("warm", None), ("cold", scratch.zero_))
    for model in a.models.split(","):
        layout = ParamLayout.from_module(build_model(model, 100))
        n = layout.param_numel
        g32 = torch.randn(n, device=dev) * 1e-3
        g16 = g32.half()
        src, dst = torch.randn(3 * n, device=dev), torch.empty(3 * n, device=dev)
        tk = T.TopKCodec(n, 0.01, dev)
        for rank in [int(r) for r in a.ranks.split(",")]:
            enc = PS.PowerSGDCodec(layout, rank, dev)
            tb = enc.table
            say(f"{model}, rank {rank}: n = {n}, {len(tb.comp)} of {len(tb.seg)} tensors compressed, payload "
                f"{tb.payload_bytes / 1e6:.3f} MB ({tb.payload_bytes / n:.4f} B/param), fp16 wire {2 * n / 1e6:.2f} MB")
            pays = []
            for w in range(max(int(w) for w in a.workers.split(","))):
                other = PS.PowerSGDCodec(layout, rank, dev, worker=w)
                pays.append(other.encode(torch.randn(n, device=dev) * 1e-3).clone())
            out = torch.zeros(n, device=dev)
            fns = {"encode, fp32 g (4 launches)": (lambda: enc.encode(g32), 24 * n),
                   "encode, fp16 g (4 launches)": (lambda: enc.encode(g16), 22 * n),
                   "topk_encode 1%, fp32 g": (lambda: tk.encode(g32), 0),
                   "copy of 24 B/param": (lambda: dst.copy_(src), 24 * n)}
            for W in [int(w) for w in a.workers.split(",")]:
                fns[f"psgd_decode, W = {W}"] = (lambda W=W: PS.decode(pays[:W], out, layout, rank), 4 * n)
            fns["copy of 4 B/param"] = (lambda: dst[:n // 2].copy_(src[:n // 2]), 4 * n)
            for mode, scrub in modes:
                t = time_alternating({k: f for k, (f, _) in fns.items()}, a.groups, a.per_group, scrub)
                per_byte = {24 * n: t["copy of 24 B/param"] / (24 * n), 4 * n: t["copy of 4 B/param"] / (4 * n)}
                say(f"  [{mode}]")
                for k, (_, nb) in fns.items():
                    if not nb:
                        say(f"    {k:32s} {t[k]:9.1f} us")
                        continue
                    ref = per_byte[24 * n] if nb > 4 * n else per_byte[4 * n]
                    say(f"    {k:32s} {t[k]:9.1f} us  {nb / 1e6:7.1f} MB  {nb / t[k] / 1e6:5.2f} TB/s  "
                        f"{t[k] / (ref * nb):5.2f} x the copy's time for these bytes")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
