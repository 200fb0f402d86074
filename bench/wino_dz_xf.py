"""The merged backward transform of the three-launch Winograd layers (csrc/kernels/wino.hip
wino_dz_xf_kernel) next to the launches it replaces, per layer shape of the fp32 ResNet-18 step at
batch 128 (8x8x256, 4x4x512), plain and with the BN-backward apply folded in (rounded as the
apply pass, as the engine runs it). The transforms it
replaces have no entry of their own, so each is the difference of two chains on one stream:
wino_wgrad - wino_wgrad_pre (the dy transform), wino_conv - wino_conv_pre (the data gradient's
input transform); the BN-backward apply (bn_bwd_apply_fin) is timed directly. One JSON line per
shape and kind, microseconds (medians of REPS timed batches; spread of the merged kernel's).

  python bench/wino_dz_xf.py [--tag NAME] [--batch B] [--reps R --iters I] [--no-det]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.ops import kernels as K  # noqa: E402

from bench.wino_fused_variants import DEV, ITERS, REPS, t_us  # noqa: E402


def layer(B, c, hw):
    n = (B, hw, hw, c)
    dz, yb, dy, dx = (torch.randn(n, device=DEV) for _ in range(4))
    w = torch.randn(c, c, 3, 3, device=DEV) / (9 * c) ** 0.5
    ud = torch.empty(36 * c * c, device=DEV)
    K.wino_weights(w, ud, c, c, flip=True)
    nv = K.wino_v_floats(B, hw, hw, c)
    v, vx, d = (torch.zeros(nv, device=DEV) for _ in range(3))
    p = torch.empty(K.wino_p_floats(B, hw, hw, c, c), device=DEV)
    q = K.wino_wgrad_q(B, hw, hw, c, c)
    wp, g = torch.empty(36 * q * c * c, device=DEV), torch.empty(c * c * 9, device=DEV)
    nslot = K.STAT_SLOTS * (K.det_slot_scale() if K.deterministic() else 1)
    saved = torch.stack([torch.randn(c, device=DEV) * 0.2, torch.rand(c, device=DEV) * 0.5 + 0.5]).contiguous()
    bp = torch.zeros(nslot, 2, c, device=DEV)
    K.bn_bwd_reduce(dz, torch.ones_like(dz), yb, saved, bp, B * hw * hw, c)
    gamma = torch.rand(c, device=DEV) + 0.5
    coef, dgb = torch.zeros(3, c, device=DEV), torch.zeros(2, c, device=DEV)
    ctr = torch.zeros(4, dtype=torch.int32, device=DEV)
    fin = K.bn_bwd_fin(gamma, saved, coef, dgb[0].data_ptr(), dgb[1].data_ptr(), ctr.data_ptr(), B * hw * hw, 1.0, c, False)
    a = (B, hw, hw, c, c)
    fns = {
        "apply": lambda: K.bn_bwd_apply_fin(dz, None, yb, bp, fin, dy, c),
        "wgrad": lambda: K.wino_wgrad(vx, dy, d, wp, g, *a),
        "wgrad_pre": lambda: K.wino_wgrad_pre(vx, d, wp, g, *a),
        "dgrad": lambda: K.wino_conv(dy, ud, dx, None, None, v, p, *a),
        "dgrad_pre": lambda: K.wino_conv_pre(v, ud, dx, None, None, p, *a),
        "dz_plain": lambda: K.wino_dz_xf(dy, v, d, B, hw, hw, c),
        "dz_fold": lambda: K.wino_dz_xf(dz, v, d, B, hw, hw, c, bwd_in=(yb, bp, fin), as_apply=True),
    }
    keep = (dz, yb, dy, dx, w, ud, v, vx, d, p, wp, g, saved, bp, gamma, coef, dgb, ctr)
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--iters", type=int, default=ITERS)
    ap.add_argument("--no-det", action="store_true", help="float-atomic BN sums (the step runs deterministic)")
    a = ap.parse_args()
    K.set_deterministic(not a.no_det)
    torch.manual_seed(0)
    for c, hw in ((256, 8), (512, 4)):
        fns, keep = layer(a.batch, c, hw)
        t = {k: t_us(f, a.reps, a.iters) for k, f in fns.items()}
        dy_xf = t["wgrad"][0] - t["wgrad_pre"][0]
        in_xf = t["dgrad"][0] - t["dgrad_pre"][0]
        base = {"tag": a.tag, "layer": f"{hw}x{hw}x{c}", "B": a.batch}
        for kind, old, new in (("plain", dy_xf + in_xf, t["dz_plain"]), ("fold", t["apply"][0] + dy_xf + in_xf, t["dz_fold"])):
            print(json.dumps({**base, "kind": kind, "replaced_us": round(old, 2), "merged_us": round(new[0], 2),
                              "merged_spread_us": round(new[1], 2), "apply_us": round(t["apply"][0], 2),
                              "dy_xf_us": round(dy_xf, 2), "in_xf_us": round(in_xf, 2)}), flush=True)
        del fns, keep


if __name__ == "__main__":
    main()
