#!/usr/bin/env python
"""Fingerprints of the server update kernels on every dispatch path: one line per cell with the
sha256 of everything the entry may write.

Where scripts/server_update_bits.py drives a ParameterServer, this one calls the public
psx.ops.kernels entries themselves (sgd_apply, sgd_apply_multi, lars_apply_multi, lars_apply,
adamw_apply_multi, lamb_apply_multi, lamb_apply, guard_apply_multi, guard_apply, dc_apply),
crossed with the wire type (fp16 / fp32), W = 1 / 3 sources, views that are 16-byte aligned or
start one element later, momentum 0 / 0.9 with weight decay (AdamW and LAMB: weight decay off /
on), the bf16 image off / on, and `first` where the entry has it. The guard takes one round that
is clipped and one with an inf in a wire; dc_apply takes the constant and the adaptive form, with
and without a backup. Two runs of the same code print the same lines; a refactor of the kernels
prints the lines of its parent (profiles/update_kernels_shared.txt holds both).

    python scripts/update_kernel_bits.py

Inputs are made on the host from one seed. Sizes are the smallest that reach every branch: the
flat kernels see n = 2 * 8192 + 8 + 5 elements (a second chunk, whole groups of 8 and a tail); the
LARS / LAMB table has three tensors of 5, 8192 + 13 and 24 elements, the middle one starting off
the 8-element grid (a head, a second chunk, a tail), the last one 1-D (not adapted), the first one
shorter than a group. A dense entry (lars_apply, lamb_apply, guard_apply) is fed the fp32 sum of
the same W wires, formed on the host in the kernels' order.
"""
import hashlib
import itertools
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import psx  # noqa: E402,F401
from psx.models.layout import Entry, ParamLayout  # noqa: E402
from psx.ops import kernels as K  # noqa: E402

DEV = "cuda"
CHUNK = 8192
N_FLAT = 2 * CHUNK + 8 + 5
TABLE = [("w5", 5, 2), ("w8205", CHUNK + 13, 2), ("b24", 24, 1)]  # (name, numel, ndim)
N_TABLE = sum(t[1] for t in TABLE)
LR, GS_SCALE, MOMENTUM, WD, ADAM_WD, ADAM_T = 0.05, 1.0, 0.9, 5e-4, 0.01, 3
DC_LAMBDA = 0.04

SGD_TAIL = ("sgd_apply", "sgd_apply_multi", "lars_apply_multi", "lars_apply", "guard_apply_multi", "guard_apply",
            "dc_apply")
ADAM = ("adamw_apply_multi", "lamb_apply_multi", "lamb_apply")
ENTRIES = SGD_TAIL[:4] + ADAM + SGD_TAIL[4:]
ON_TABLE = ("lars_apply_multi", "lars_apply", "lamb_apply_multi", "lamb_apply")
DENSE_OF = {"lars_apply_multi": "lars_apply", "lamb_apply_multi": "lamb_apply", "guard_apply_multi": "guard_apply"}
VARIANTS = {"guard_apply_multi": ("clip", "inf"), "guard_apply": ("clip", "inf"),
            "dc_apply": ("const_bak", "const_nobak", "adapt_bak", "adapt_nobak")}

# mom: momentum 0.9 and weight decay on the SGD-tail entries, weight decay alone on AdamW / LAMB
Cell = namedtuple("Cell", "entry wire W off mom first img var")


def cells():
    for entry in ENTRIES:
        ws = (1,) if entry in ("sgd_apply", "dc_apply") else (1, 3)
        firsts = (0, 1) if entry in SGD_TAIL else (0,)
        for wire, W, off, mom, first, img, var in itertools.product(("fp16", "fp32"), ws, (0, 1), (0, 1), firsts,
                                                                    (0, 1), VARIANTS.get(entry, ("-",))):
            if first and not mom:  # `first` is read with momentum only
                continue
            yield Cell(entry, wire, W, off, mom, first, img, var)


def table_layout() -> ParamLayout:
    lay = ParamLayout()
    off = 0
    for name, numel, ndim in TABLE:
        lay.entries[name] = Entry(name, (numel, 1) if ndim > 1 else (numel,), "float32", "param", off, numel)
        off += numel
    lay.param_numel = off
    return lay


def host_inputs():
    """Everything a cell reads, made once on the host from one seed (N_FLAT elements; the table
    entries take the first N_TABLE)."""
    gen = torch.Generator().manual_seed(4321)
    r = lambda: torch.randn(N_FLAT, generator=gen)  # noqa: E731
    h = dict(p=r() * 0.1, buf=r() * 0.01, m=r() * 0.01, v=r().square() * 1e-4, ms=r().square() * 1e-4)
    h["bak"] = h["p"] + r() * 0.01
    h["g"] = [r() * 0.01 for _ in range(3)]
    return h


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def view(src, off, dtype=None):
    """A device copy of the host tensor as a view that starts `off` elements into its allocation
    (off 0: 16-byte aligned; 1: no 16-byte access possible)."""
    src = src if dtype is None else src.to(dtype)
    buf = torch.zeros(src.numel() + off, dtype=src.dtype, device=DEV)
    buf[off:].copy_(src)
    return buf[off:]


def wire_sum(gs):
    """The fp32 sum of the decoded wires as the kernels form it: from 0, in source order."""
    s = torch.zeros_like(gs[0], dtype=torch.float32)
    for g in gs:
        s += g.float()
    return s


def run_cell(c: Cell, H, lay=None, dense_sum=False) -> dict:
    """Run one cell on fresh device copies of the host inputs H; returns {written tensor: sha}.
    dense_sum: a multi-source entry is handed the fp32 host sum of its wires as its one source."""
    n = N_TABLE if c.entry in ON_TABLE else N_FLAT
    wdt = torch.float16 if c.wire == "fp16" else torch.float32
    gs = [g[:n].to(wdt) for g in H["g"][:c.W]]
    if c.var == "inf":
        gs[0] = gs[0].clone()
        gs[0][7] = float("inf")
    d = lambda k: view(H[k][:n], c.off)  # noqa: E731
    p = d("p")
    img = view(torch.zeros(n, dtype=torch.bfloat16), c.off) if c.img else None
    out = {"p": p, "img": img}
    gscale = GS_SCALE / c.W
    if c.entry in SGD_TAIL:
        buf = d("buf") if c.mom else None
        sgd = dict(gscale=gscale, momentum=MOMENTUM if c.mom else 0.0, wd=WD if c.mom else 0.0, buf=buf,
                   first=bool(c.first), n=n, img=img)
        out["buf"] = buf
    else:
        m, v = d("m"), d("v")
        adam = dict(gscale=gscale, wd=ADAM_WD if c.mom else 0.0, n=n, img=img)
        out.update(m=m, v=v)
    srcs = [view(g, c.off) for g in ([wire_sum(gs)] if dense_sum else gs)]
    dense = c.entry in DENSE_OF.values()
    if dense or c.entry in DENSE_OF:
        stage = view(wire_sum(gs) if dense else torch.zeros(n), c.off)
        out["stage"] = stage
    if c.entry in ON_TABLE:
        tab = K.LarsTable(lay or table_layout(), DEV)
        out["ratios"] = tab.ratios
    if c.entry.startswith("guard"):
        st = K.GuardState(n, DEV)
        s = wire_sum(gs).double()
        clip = 0.5 * gscale * float(s.norm()) if c.var == "clip" else 0.0
        out["state"] = st.state

    if c.entry == "sgd_apply":
        K.sgd_apply(p, srcs[0], LR, **sgd)
    elif c.entry == "sgd_apply_multi":
        K.sgd_apply_multi(p, srcs, LR, **sgd)
    elif c.entry == "lars_apply_multi":
        K.lars_apply_multi(p, srcs, stage, tab, LR, **sgd)
    elif c.entry == "lars_apply":
        K.lars_apply(p, stage, tab, LR, **sgd)
    elif c.entry == "adamw_apply_multi":
        K.adamw_apply_multi(p, srcs, m, v, LR, ADAM_T, **adam)
    elif c.entry == "lamb_apply_multi":
        K.lamb_apply_multi(p, srcs, stage, m, v, tab, LR, ADAM_T, **adam)
    elif c.entry == "lamb_apply":
        K.lamb_apply(p, stage, m, v, tab, LR, ADAM_T, **adam)
    elif c.entry == "guard_apply_multi":
        K.guard_apply_multi(p, srcs, stage, st, LR, clip_norm=clip, **sgd)
    elif c.entry == "guard_apply":
        K.guard_apply(p, stage, st, LR, clip_norm=clip, **sgd)
    else:  # dc_apply
        form, backup = c.var.split("_")
        ms = d("ms") if form == "adapt" else None
        out["ms"] = ms
        K.dc_apply(p, srcs[0], d("bak") if backup == "bak" else None, LR, DC_LAMBDA, ms=ms, **sgd)
    torch.cuda.synchronize()
    if c.entry.startswith("guard"):
        r = st.read()
        assert r["skip"] == (c.var == "inf") and (c.var != "clip" or r["coef"] < 1.0), (c, r)
    return {k: sha(t) for k, t in out.items() if t is not None}


def label(c: Cell) -> str:
    return f"{c.entry} wire={c.wire} W={c.W} off={c.off} mom={c.mom} first={c.first} img={c.img} var={c.var}"


def main():
    H, lay = host_inputs(), table_layout()
    count = 0
    for c in cells():
        print(label(c), " ".join(f"{k}={v}" for k, v in run_cell(c, H, lay).items()), flush=True)
        count += 1
    print(f"# {count} cells, n = {N_FLAT} (flat) / {N_TABLE} (table)", flush=True)


if __name__ == "__main__":
    main()
