#!/usr/bin/env python3
"""Is the gfx950 code of csrc/kernels/*.hip files the same in two source trees? For refactors that
must not change a kernel: each file is compiled device-only to assembly in both trees, each with
its own tree's build flags (csrc/build.py kernel_flags, FILE_FLAGS included), no GPU needed, and
the compiler's text is compared per symbol.

  git worktree add --detach /tmp/parent HEAD~1
  python scripts/prof/isa_equal.py /tmp/parent . conv_v2.hip wino_fused.hip [-j N]

This is a plain text comparison: nothing inside the assembly is interpreted. The only
normalisation is the compilation-unit id, a hash of the source text that names one symbol
(__hip_cuid_<hash>). One line per file (symbols, kernels among them, how many differ) and one per
differing symbol; exit status 1 on any difference.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
FUNC = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
TAIL_AT = re.compile(r"^\s*\.(type\s+[^\s,]+,@object|amdgpu_metadata)\b")
LEAD = re.compile(r"^\s*\.(section|protected|globl|weak|hidden|p2align)\b")
HEAD, TAIL ="<head>", "<tail>"


def normalise(text: str) -> str:
    return CUID.sub("__hip_cuid_", text)


def split_symbols(text: str) -> tuple[dict, set]:
    """{symbol: its text} of one assembly file, and the set of symbols that are kernels. A
    symbol's text runs from its '.type S,@function' line to the next one: the code, for a kernel
    the descriptor that follows it (.amdhsa_kernel .. .end_amdhsa_kernel, the register and LDS
    budget) and the compiler's resource comments. What precedes the first symbol is HEAD; from the
    first variable ('.type V,@object') or the metadata note on, all is TAIL. The directives right in
    front of a '.type' line (.section / .protected / .globl / .p2align ...) name the symbol that
    follows and go with it, so symbols compare equal in whatever order the two files define them."""
    parts, kernels, name = {HEAD: []}, set(), HEAD
    for line in text.splitlines():
        m = FUNC.match(line)
        if name != TAIL and m:
            prev, name = parts[name], m.group(1)
            if name in parts:
                raise ValueError(f"symbol {name} defined twice")
            n = len(prev)
            while n and LEAD.match(prev[n - 1]):
                n -= 1
            parts[name] = prev[n:]
            del prev[n:]
        elif name != TAIL and TAIL_AT.match(line):
            name = TAIL
            parts[name] = []
        m = KERNEL.match(line)
        if m:
            kernels.add(m.group(1))
        parts[name].append(line)
    return {k: "\n".join(v) for k, v in parts.items()}, kernels


def compare(a: str, b: str) -> tuple[int, int, list]:
    """(symbols, kernels among them, names whose text differs or that one side lacks) of two
    assembly texts; HEAD and TAIL are compared too but not counted as symbols."""
    pa, ka = split_symbols(normalise(a))
    pb, kb = split_symbols(normalise(b))
    names = sorted(set(pa) | set(pb))
    nsym = sum(n not in (HEAD, TAIL) for n in names)
    return nsym, len(ka | kb), [n for n in names if pa.get(n) != pb.get(n)]


def _build_mod(tree: str):
    spec = importlib.util.spec_from_file_location("_psx_build", os.path.join(tree, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(tree: str, name: str) -> str:
    b = _build_mod(tree)
    src = os.path.join(os.path.abspath(tree), "csrc", "kernels", name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [b.HIPCC] + b.kernel_flags(["-O3"], src) + ["--cuda-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("command failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stdout))
        with open(out) as f:
            return f.read()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("names", nargs="+", help="file names under csrc/kernels/")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args(argv)
    names = [os.path.basename(n) for n in a.names]
    with cf.ThreadPoolExecutor(max_workers=max(1, a.j)) as ex:
        texts = list(ex.map(lambda tn: assembly(*tn), [(t, n) for n in names for t in (a.tree_a, a.tree_b)]))
    bad = 0
    for i, n in enumerate(names):
        nsym, nker, diff = compare(texts[2 * i], texts[2 * i + 1])
        print(f"{n}: {nsym} symbols ({nker} kernels), {len(diff)} differ")
        for d in diff:
            print(f"  DIFFERENT {d}")
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
