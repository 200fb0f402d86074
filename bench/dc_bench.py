"""Delay-compensated update timing (csrc/kernels/dcasgd.hip) against the SGD update it replaces.

  python bench/dc_bench.py [--models resnet18,resnet50] [--groups 20] [--per-group 10]

On the parameter counts of the models, one fp16 wire, the bf16 image on: the device time of
dc_apply in its constant and adaptive forms next to psx_sgd_apply with the same momentum and
weight decay, in the same process, the three alternating; without momentum and with momentum 0.9.
Each figure comes with the bytes the kernel must move per parameter

  sgd_apply          : 2 (g) + 4 (w read) + 4 (w written) + 2 (image)          = 12   [+ 8 momentum]
  dc_apply, constant : the same + 4 (backup read)                              = 16   [+ 8 momentum]
  dc_apply, adaptive : the same + 4 (mean square read) + 4 (mean square written) = 24 [+ 8 momentum]

the resulting rate, and that rate as a fraction of a streaming fp32 copy of the same size measured
here the same way (warm: back-to-back launches on buffers that stay in the Infinity Cache; cold:
a 512 MiB scrub before every launch; see bench/q8_bench.py for the two schemes). Without momentum
the byte counts give the expectation the run is checked against: constant <= 16/12 x the SGD time
x 1.10, adaptive <= 24/12 x the SGD time x 1.10 (10 %: box-to-box movement of ~5 % on 20-60 us
launches); a miss is printed as a miss.

Then dc_fetch_copy (the fetch that leaves the backup: 4 read + 8 written per parameter) against
the two device copies it replaces (8 read + 8 written).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dc_bench measures device time: it needs the GPU"
    dev = "cuda"
    scratch = torch.zeros(512 << 18, dtype=torch.float32, device=dev)  # 512 MiB
    wd, lr, lam = 5e-4, 1e-6, 2.0
    for model in a.models.split(","):
        lay = ParamLayout.from_module(build_model(model, 100))
        n, na = lay.param_numel, lay.arena_numel
        print(f"{model}: n = {n} trainable parameters, arena {na}", flush=True)
        src, dst = torch.randn(n, device=dev), torch.empty(n, device=dev)
        copy = {}
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            us = time_alternating({"copy": lambda: dst.copy_(src)}, a.groups, a.per_group, scrub)["copy"]
            copy[mode] = 8 * n / us / 1e6
            print(f"[{mode}] streaming fp32 copy: {us:.1f} us, {copy[mode]:.2f} TB/s", flush=True)
        g = (torch.randn(n, device=dev) * 1e-3).half()
        for mom in (0.0, 0.9):
            st = {k: dict(p=torch.randn(n, device=dev) * 0.05, img=torch.zeros(n, dtype=torch.bfloat16, device=dev),
                          buf=torch.zeros(n, device=dev) if mom else None) for k in ("sgd", "const", "adapt")}
            bak = st["const"]["p"] + 1e-3 * torch.randn(n, device=dev)
            bak2 = st["adapt"]["p"] + 1e-3 * torch.randn(n, device=dev)
            ms = torch.zeros(n, device=dev)
            kw = dict(gscale=0.5, momentum=mom, wd=wd, n=n)
            fns = {"sgd": lambda s=st["sgd"]: K.sgd_apply(s["p"], g, lr, buf=s["buf"], img=s["img"], **kw),
                   "const": lambda s=st["const"]: K.dc_apply(s["p"], g, bak, lr, lam, buf=s["buf"], img=s["img"], **kw),
                   "adapt": lambda s=st["adapt"]: K.dc_apply(s["p"], g, bak2, lr, lam, ms=ms, buf=s["buf"],
                                                             img=s["img"], **kw)}
            extra = 8 if mom else 0
            for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
                print(f"[{mode}] server update, fp16 wire, bf16 image, momentum {mom}, weight decay {wd}", flush=True)
                t = time_alternating(fns, a.groups, a.per_group, scrub)
                report("sgd_apply", t["sgd"], n * (12 + extra), copy[mode])
                report("dc_apply constant", t["const"], n * (16 + extra), copy[mode])
                report("dc_apply adaptive", t["adapt"], n * (24 + extra), copy[mode])
                for k, b in (("const", 16 + extra), ("adapt", 24 + extra)):
                    bound = b / (12 + extra) * 1.10
                    r = t[k] / t["sgd"]
                    print(f"  dc {k} / sgd time: {r:.3f}  (bytes {b}/{12 + extra} x 1.10 = {bound:.3f}: "
                          f"{'within' if r <= bound else 'MISSED'})", flush=True)
            assert all(bool(torch.isfinite(s["p"]).all()) for s in st.values())
        arena = torch.randn(na, device=dev)
        local, fb = torch.empty(na, device=dev), torch.empty(n, device=dev)
        local2, fb2 = torch.empty(na, device=dev), torch.empty(n, device=dev)

        def two_copies():
            local2.copy_(arena)
            fb2.copy_(arena[:n])

        fns = {"fused": lambda: K.dc_fetch_copy(arena, local, fb, n), "two": two_copies,
               "backup_only": lambda: K.dc_fetch_copy(arena, None, fb, n)}
        for mode, scrub in (("warm", None), ("cold", scratch.zero_)):
            print(f"[{mode}] fetch that leaves the backup", flush=True)
            t = time_alternating(fns, a.groups, a.per_group, scrub)
            report("dc_fetch_copy (arena -> worker + backup)", t["fused"], 4 * na + 4 * na + 4 * n, copy[mode])
            report("two device copies", t["two"], 8 * na + 8 * n, copy[mode])
            report("dc_fetch_copy, backup only", t["backup_only"], 8 * n, copy[mode])
            print(f"  fused / two copies time: {t['fused'] / t['two']:.3f}  (bytes 12/16 = 0.750)", flush=True)
        assert torch.equal(local, arena) and torch.equal(fb, arena[:n])


if __name__ == "__main__":
    main()
