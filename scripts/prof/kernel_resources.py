#!/usr/bin/env python3
"""Per-kernel register / spill / LDS table of one csrc/kernels/*.hip file, from the compiler's own
resource remarks (-Rpass-analysis=kernel-resource-usage): device-only compile with the build's
flags (csrc/build.py, FILE_FLAGS included), no GPU needed. One JSON line per instantiation:

  python scripts/prof/kernel_resources.py csrc/kernels/wino_fused.hip [-D NAME=VALUE ...]

Fields: vgprs, agprs, sgprs, sgpr_spills, vgpr_spills, scratch (bytes / lane), lds (bytes / block),
occupancy (waves / SIMD).
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
          "LDS Size [bytes/block]": "lds"}


def _build_mod():
    spec = importlib.util.spec_from_file_location("_psx_build", os.path.join(ROOT, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _demangle(names, hipcc):
    filt = shutil.which("llvm-cxxfilt") or os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin",
                                                        "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = shutil.which("c++filt")
    if not filt:
        raise RuntimeError("no llvm-cxxfilt or c++filt to demangle the kernel names with")
    r = subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    out = r.stdout.split("\n")[:len(names)]
    if r.returncode != 0 or len(out) != len(names):
        raise RuntimeError(f"{filt} failed on the kernel names")
    return out


def parse_remarks(text: str) -> list[dict]:
    """The remark blocks of one compile: 'Function Name: X' followed by one line per resource."""
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: (?:.*?: )?\s*Function Name: (\S+)", line)
        if m:
            cur = {"kernel": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s*([A-Za-z][A-Za-z \[\]/]*?): (-?\d+)\b", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return rows


def kernel_resources(src: str, defines=()) -> list[dict]:
    b = _build_mod()
    src = os.path.abspath(src)
    flags = b.kernel_flags(["-O3"], src) + ["--cuda-device-only"]  # the build's own flags, device side only
    flags += [d if d.startswith("-") else f"-D{d}" for d in defines]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [b.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "k.o")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stdout))
    rows = parse_remarks(r.stdout)
    for row, name in zip(rows, _demangle([x["kernel"] for x in rows], b.HIPCC)):
        row["kernel"] = re.sub(r"^void ", "", name).replace("psx::", "")
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    a = ap.parse_args(argv)
    rows = kernel_resources(a.src, a.defines)
    if not rows:
        print("no kernel-resource-usage remarks in the compiler output", file=sys.stderr)
        return 1
    for row in rows:
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
