#!/usr/bin/env python3
"""Which weight-gradient kernels does the planner reach? Asks K.conv_wgrad2_path (host code only,
no GPU needed) for every shape of a grid and prints the routes reached, the smallest shape that
takes each, and the instantiations of csrc/kernels/wgrad_v2.hip's launch tables that no shape of
the grid takes (profiles/wgrad_routes.txt is this output).

  python scripts/prof/wgrad_routes.py [--batches 1,2,...] [--channels 64,...] [--sizes 4,...]
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# the launch tables of wgrad_v2.hip (kW2fKernels, kW3fKernels, kW3Kernels, kW2Kernels)
INSTANTIATED = (["wgrad2_kernel<128,128,4>", "wgrad2_kernel<128,64,3>", "wgrad2_kernel<64,128,3>",
                 "wgrad2_kernel<64,64,3>"] +
                [f"wgrad2f_kernel<{br},{bc},3>" for br in (128, 64) for bc in (128, 64)] +
                [f"wgrad3_kernel<{bc},{ns},{g}>" for g in ("false", "true") for bc in (128, 64) for ns in (6, 3)] +
                ["wgrad3f_kernel<128,3>", "wgrad3f_kernel<64,3>"])
KINDS3 = ((3, 1, 1), (1, 1, 0), (3, 2, 1))  # (k, stride, pad)


def kernel_name(p) -> str:
    if p["kind"] == "stem7":
        return "stem7_wgrad_kernel (stem.hip)"
    if p["kind"] == "tile":
        return f"wgrad2f_kernel<{p['br']},{p['bc']},{p['ns']}>" if p["f32"] else \
            f"wgrad2_kernel<{p['br']},{p['bc']},{p['ns']}>"
    if p["f32"]:
        return f"wgrad3f_kernel<{p['bc']},{p['ns']}>"
    return f"wgrad3_kernel<{p['bc']},{p['ns']},{'true' if p['kind'] == 'tap_reuse_general' else 'false'}>"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,2,3,4,6,8,12,16,24,32,48,64,96,128")
    ap.add_argument("--channels", default="64,128,256,512")
    ap.add_argument("--sizes", default="4,8,16,32,7,14,28")
    a = ap.parse_args(argv)
    batches, chans, sizes = ([int(v) for v in s.split(",")] for s in (a.batches, a.channels, a.sizes))

    import psx  # noqa: F401
    from psx.ops import kernels as K

    # shape: (n, ic, oc, hw, k, stride, pad, f32); the ImageNet stem (fp32: its own kernel) rides along
    shapes = [(n, ic, oc, hw, k, s, p, f32) for n, ic, oc, hw, (k, s, p), f32 in
              itertools.product(batches, chans, chans, sizes, KINDS3, (False, True))]
    shapes += [(n, 4 if f32 else 8, 64, 224, 7, 2, 3, f32) for n in batches for f32 in (False, True)]
    reached, refused = {}, 0
    for sh in shapes:
        n, ic, oc, hw, k, s, p, f32 = sh
        path = K.conv_wgrad2_path(n, hw, hw, ic, oc, k, s, p, -(-(k * k * ic) // 64) * 64, f32)
        if not isinstance(path, dict):
            refused += 1
            continue
        oh = (hw + 2 * p - k) // s + 1
        work = n * oh * oh * ic * oc * k * k
        cnt, best = reached.get(kernel_name(path), (0, None))
        reached[kernel_name(path)] = (cnt + 1, min(best, (work, sh, path["splits"])) if best else (work, sh, path["splits"]))

    print("grid: batch {%s} x in-channels {%s} x out-channels {%s} x H=W {%s}" % (a.batches, a.channels, a.channels,
                                                                                 a.sizes))
    print("      x {3x3/s1/p1, 1x1/s1/p0, 3x3/s2/p1} x {bf16, fp32}, plus the ImageNet stem (3 -> 64, 7x7/s2, 224)")
    print(f"      {len(shapes)} shapes, {refused} refused, {len(reached)} distinct routes reached\n")
    print("routes reached (shapes of the grid that take it; smallest such shape as")
    print("batch x in-channels x out-channels x H=W, kernel/stride, dtype -> its split count):")
    for name in sorted(reached):
        cnt, (_, (n, ic, oc, hw, k, s, p, f32), splits) = reached[name]
        print(f"  {name:34s} {cnt:6d}   {n}x{ic}x{oc}x{hw}, {k}x{k}/s{s}, {'fp32' if f32 else 'bf16'} -> {splits} splits")
    print("\ninstantiated, but taken by no shape of the grid:")
    for name in INSTANTIATED:
        if name not in reached:
            print(f"  {name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
