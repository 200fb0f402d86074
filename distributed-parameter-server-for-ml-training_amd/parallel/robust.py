"""Byzantine-robust aggregation of a sync round's gathered dense wires (--aggregate trimmed /
median / krum): what ParameterServer.update_range puts in front of its rule in place of the fp32
sum of the wires.

``x_(0) <= ... <= x_(W-1)`` are the W decoded values of one coordinate, sorted, NaN counted as +inf.

* trimmed: e = (sum_{r=T}^{W-1-T} x_(r)) * fl(1 / (W - 2T)), the sum in fp32 in rank order from 0
  (--trim T; W > 2T);
* median: e = x_((W-1)/2) for odd W, 0.5 * (x_(W/2-1) + x_(W/2)) in fp32 for even W;
* krum: multi-Krum (Blanchard et al. 2017; --byzantine F; W >= 2F + 3). G_ij = <g_i, g_j> over the
  whole arena, d2_ij = G_ii + G_jj - 2 G_ij (non-finite: +inf), score_i = the sum of the W-F-2 smallest
  d2_ij with j != i; the m = W-F workers with the smallest score are selected (ties: the lower index;
  a non-finite score ranks last); e = (the fp32 sum of the selected wires in source order) * fl(1 / m).

trimmed and median sum in rank order, so they do not depend on the order of the workers in the list.

Device: csrc/kernels/robust.hip, one launch for trimmed / median (a register sorting network per
lane), three for krum (the Gram matrix on MFMA, the selection in one workgroup, the selected sum);
no host synchronisation: the per-worker selection counters stay in a device block that
``metrics`` reads once. CPU arena: ``combine_host``, the same definitions in torch.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K

KINDS = ("trimmed", "median", "krum")


def min_sources(kind: str, trim: int = 1, byzantine: int = 1) -> int:
    """The fewest sources the rule is defined for."""
    return {"trimmed": 2 * trim + 1, "median": 1, "krum": 2 * byzantine + 3}[kind]


def check_sources(W: int, kind: str, trim: int = 1, byzantine: int = 1):
    need = min_sources(kind, trim, byzantine)
    if W < need:
        knob = {"trimmed": f"--trim {trim}", "median": "", "krum": f"--byzantine {byzantine}"}[kind]
        raise ValueError(f"--aggregate {kind} {knob} needs at least {need} sources, this round has {W} (after an elastic "
                         f"shrink or with --sync-semantics reference a round can be short); there is no fall-back to "
                         f"the mean")


def krum_select_host(X: torch.Tensor, byzantine: int) -> torch.Tensor:
    """The bool [W] selection of multi-Krum from the wires X [W, n] (Gram matrix in double)."""
    W = X.shape[0]
    Xd = X.double()
    G = Xd @ Xd.t()
    g = G.diagonal()
    d2 = g[:, None] + g[None, :] - 2.0 * G
    d2 = torch.where(torch.isfinite(d2), d2, torch.full_like(d2, float("inf")))
    d2.fill_diagonal_(float("inf"))  # j != i: the diagonal sorts past the W - 1 others
    score = torch.sort(d2, dim=1, stable=True).values[:, : W - byzantine - 2].sum(1)
    score = torch.where(torch.isfinite(score), score, torch.full_like(score, float("inf")))
    sel = torch.zeros(W, dtype=torch.bool)
    sel[torch.sort(score, stable=True).indices[: W - byzantine]] = True
    return sel


def combine_host(srcs: list, n: int, kind: str, trim: int = 1, byzantine: int = 1, c: float = 1.0, out=None):
    """The estimate of the sources' first n elements times fl(c), in torch fp32 (the module
    docstring's definitions). Returns (out fp32 [n], the bool [W] selection of krum or None)."""
    W = len(srcs)
    check_sources(W, kind, trim, byzantine)
    X = torch.stack([s[:n].to(torch.float32) for s in srcs])
    sel = None
    if kind == "krum":
        sel = krum_select_host(X, byzantine)
        e = torch.zeros(n, dtype=torch.float32)
        for k in range(W):
            if sel[k]:
                e = e + X[k]
        e = e * float(np.float32(1.0) / np.float32(W - byzantine))
    else:
        S = torch.sort(torch.where(torch.isnan(X), torch.full_like(X, float("inf")), X), dim=0).values
        if kind == "median":
            e = S[(W - 1) // 2] if W % 2 else 0.5 * (S[W // 2 - 1] + S[W // 2])
        else:
            e = torch.zeros(n, dtype=torch.float32)
            for r in range(trim, W - trim):
                e = e + S[r]
            e = e * float(np.float32(1.0) / np.float32(W - 2 * trim))
    e = e * float(np.float32(c))
    if out is None:
        return e, sel
    out[:n].copy_(e)
    return out, sel


class Robust:
    """The robust combine of one server: its configuration, the round count and, for krum, the
    device scratch and selection counters (ops/kernels.py KrumState) or their host counterpart."""

    def __init__(self, cfg, n: int, device):
        self.kind, self.trim, self.byzantine = cfg.aggregate, int(cfg.trim), int(cfg.byzantine)
        self.n, self.device = n, torch.device(device)
        self.rounds = 0
        self._krum = self._host_selected = None
        if self.kind == "krum":
            if self.device.type == "cuda":
                self._krum = K.KrumState(n, self.device)
            else:
                self._host_selected = [0] * 32

    def combine(self, srcs: list, out: torch.Tensor, weight: float, whole: bool) -> torch.Tensor:
        """out = e * c from the W unsummed dense wires (each holding the range in its first
        out.numel() elements), c = fl(1 / fl(weight)): the rule that follows multiplies its one
        already-summed source by ``weight``, so it applies the estimate e where weight is 1 / W, and
        any other weight (reference semantics) keeps its meaning as a scale on e."""
        W, n = len(srcs), out.numel()
        check_sources(W, self.kind, self.trim, self.byzantine)
        if self.kind == "krum" and not whole:
            raise ValueError(f"--aggregate krum scores the workers over the whole gradient: a partial range of {n} of "
                             f"{self.n} elements cannot be combined (no bucketed or sharded updates)")
        c = float(np.float32(1.0) / np.float32(weight))
        srcs = [s if s.numel() == n else s[:n] for s in srcs]
        self.rounds += 1
        if self.device.type != "cuda":
            _, sel = combine_host(srcs, n, self.kind, self.trim, self.byzantine, c, out)
            if sel is not None:
                self._host_selected = [a + int(b) for a, b in zip(self._host_selected, sel.tolist() + [0] * (32 - W))]
        elif self.kind == "krum":
            K.robust_gram(srcs, self._krum)
            K.robust_krum_select(self._krum, W, self.byzantine)
            K.robust_select_sum(srcs, self._krum, out, W - self.byzantine, c)
        else:
            K.robust_rank(srcs, out, self.kind, self.trim, c, n=n)
        return out

    def metrics(self, workers: int) -> dict:
        m = {"kind": self.kind, "rounds": int(self.rounds)}
        if self.kind == "trimmed":
            m["trim"] = self.trim
        if self.kind == "krum":
            m["byzantine"] = self.byzantine
            sel = self._krum.selected.cpu().tolist() if self._krum is not None else self._host_selected
            m["krum_selected_per_worker"] = [int(v) for v in sel[:workers]]
        return m
