"""Each wino_fused_kernel instantiation the fp32 ResNet-18 step launches (csrc/kernels/wino_fused.hip),
timed alone at batch 128: the 32x32x64 and 16x16x128 layers, forward (plain input / the previous
layer's BN + ReLU folded in, BN slot sums, no V side output — the engine's fused weight gradient
needs none) and the data-gradient epilogues of the step (mask from o + residual, mask from the
affine, two BNs + residual), each with a plain input and with the BN-backward apply folded into the
operand loads. One JSON line per variant, microseconds (median of REPS timed batches and their
spread); PSX_KERNELS_LIB selects the kernel library, as in every A/B here.

  python bench/wino_fused_variants.py [--tag NAME] [--build LABEL] [--reps R --iters I]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.ops import kernels as K  # noqa: E402

DEV = "cuda"
REPS, ITERS = 7, 20


def t_us(fn, reps=REPS, iters=ITERS):
    for _ in range(5):
        fn()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(1e3 * s.elapsed_time(e) / iters)
    return statistics.median(out), max(out) - min(out)


def variants(B, c, hw):
    """(name, template arguments <G, RES, BWD, MAFF, TWO>, input kind, launch)."""
    n = (B, hw, hw, c)
    x = torch.relu(torch.randn(n, device=DEV))
    z = torch.empty(n, device=DEV)
    dy, res = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    o, y1, y2, yb = (torch.randn(n, device=DEV) for _ in range(4))
    w = torch.randn(c, c, 3, 3, device=DEV) / (9 * c) ** 0.5
    uf, ufd = torch.empty(40 * c * c, device=DEV), torch.empty(40 * c * c, device=DEV)
    K.WinoWeightBatch([(w, uf, c, c, False, 1), (w, ufd, c, c, True, 1)])()
    y, dx = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    nslot = K.STAT_SLOTS * (K.det_slot_scale() if K.deterministic() else 1)
    stats = torch.zeros(nslot, 2, c, device=DEV)
    part = torch.zeros(nslot, 3, c, device=DEV)
    ssh = torch.randn(c, device=DEV) * 0.1
    cnt = B * hw * hw
    t = {k: torch.rand(c, device=DEV) + 0.5 for k in ("gamma", "beta", "rm", "rv")}
    ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
    # folded forward BN of the input, as the engine feeds it: z is a conv's pre-BN output and sl the
    # slot sums that launch produced (shifted around zsh)
    zsh = torch.zeros(c, device=DEV)
    sl = torch.zeros(nslot, 2, c, device=DEV)
    K.wino_fused(x, uf, z, None, sl, None, B, hw, hw, c, c, sshift=zsh)
    aff, sav = torch.zeros(2, c, device=DEV), torch.zeros(2, c, device=DEV)
    fin = K.bn_fin(t["gamma"], t["beta"], t["rm"], t["rv"], aff, sav, ctr.data_ptr(), cnt, 1e-5, 0.1, c, sshift=zsh,
                   sshift_next=torch.zeros(c, device=DEV))
    # folded BN backward of the data gradient's input: dz and the backward slot sums bp of the BN
    # whose forward input is yb, from a data-gradient launch with that BN as its consumer
    saved = torch.stack([torch.randn(c, device=DEV) * 0.2, torch.rand(c, device=DEV) * 0.5 + 0.5]).contiguous()
    dz = torch.empty(n, device=DEV)
    bp = torch.zeros(nslot, 2, c, device=DEV)
    K.wino_fused(dy, ufd, dz, None, None, None, B, hw, hw, c, c,
                 bst=K.bwd_stats_desc(bp, o, yb, saved, mask_store=True))
    coef, dgb = torch.zeros(3, c, device=DEV), torch.zeros(2, c, device=DEV)
    bfin = K.bn_bwd_fin(t["gamma"], saved, coef, dgb[0].data_ptr(), dgb[1].data_ptr(), ctr.data_ptr(), cnt, 1.0, c,
                        False)
    maff = torch.stack([torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)]).contiguous()
    sv1, sv2 = saved.clone(), saved.clone()
    b_o = K.bwd_stats_desc(part, o, y1, sv1, mask_store=True)
    b_a = K.bwd_stats_desc(part, None, y1, sv1, mask_store=True, mask_aff=maff)
    b_2 = K.bwd_stats_desc(part, o, y1, sv1, y2, sv2, mask_store=True)
    keep = (x, z, dy, dz, res, o, y1, y2, yb, uf, ufd, y, dx, stats, part, ssh, t, zsh, sl, aff, sav, ctr, saved, bp, coef,
            dgb, maff, sv1, sv2)
    G = c // 16

    def fwd(bn_in):
        src = z if bn_in else x
        return lambda: K.wino_fused(src, uf, y, None, stats, None, B, hw, hw, c, c, bn_in=(sl, fin) if bn_in else None,
                                    sshift=ssh)

    def dgrad(bst, r, fold):
        return lambda: K.wino_fused(dz if fold else dy, ufd, dx, res if r else None, None, None, B, hw, hw, c, c, bst=bst,
                                    bwd_in=(yb, bp, bfin) if fold else None)

    out = [("fwd", (G, 0, 0, 0, 0), "plain", fwd(False)), ("fwd", (G, 0, 0, 0, 0), "bnin", fwd(True))]
    dg = [("dgrad_maff", (G, 0, 1, 1, 0), b_a, False)]
    dg.append(("dgrad_res_o", (G, 1, 1, 0, 0), b_o, True) if c == 64 else ("dgrad_res_two", (G, 1, 1, 0, 1), b_2, True))
    for name, targs, bst, r in dg:
        for fold in (False, True):
            out.append((name, targs, "bwdin" if fold else "plain", dgrad(bst, r, fold)))
    return out, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default=os.environ.get("PSX_KERNELS_LIB", "tree"))
    ap.add_argument("--build", default="", help="free-text label of the library under test, copied into every line")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--iters", type=int, default=ITERS, help="launches per timed batch (few under a profiler)")
    ap.add_argument("--no-det", action="store_true", help="float-atomic BN sums (the step runs deterministic)")
    a = ap.parse_args()
    K.set_deterministic(not a.no_det)
    torch.manual_seed(0)
    for c, hw in ((64, 32), (128, 16)):
        vs, keep = variants(a.batch, c, hw)
        for name, targs, kind, fn in vs:
            med, spread = t_us(fn, a.reps, a.iters)
            print(json.dumps({"tag": a.tag, **({"build": a.build} if a.build else {}), "layer": f"{hw}x{hw}x{c}", "B": a.batch, "variant": name,
                              "template": "<%d, %s>" % (targs[0], ", ".join("true" if v else "false" for v in targs[1:])),
                              "input": kind, "us": round(med, 2), "spread_us": round(spread, 2)}), flush=True)
        del vs, keep


if __name__ == "__main__":
    main()
