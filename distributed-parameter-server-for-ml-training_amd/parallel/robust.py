"""Byzantine-robust aggregation of a sync round's gathered dense wires (--aggregate trimmed /
median / krum / geomed / cclip): what ParameterServer.update_range puts in front of its rule in place of the fp32
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

The two iterative whole-vector rules (--aggregate geomed / cclip). ``g_k`` is wire k decoded to fp32,
k = 0..W-1; ``d_k(v) = sqrt(sum_i (g_k[i] - v[i])^2)``, a non-finite d_k^2 counting as +inf. Both need
W >= 3 and the whole gradient.

* geomed: the geometric median by smoothed Weiszfeld steps (RFA, Pillutla et al. 2019; --robust-iters
  L, --geomed-eps nu). v_0 = 0, so the first distances are the wires' norms and a huge or non-finite
  wire is down-weighted from step 1 on. For t = 1..L: w_k = 1 / max(d_k(v_{t-1}), nu), 0 where d_k =
  +inf; a_k = fl32(w_k / sum_j w_j); v_t = sum_k a_k g_k. e = v_L.
* cclip: centred clipping (Karimireddy, He, Jaggi 2021; --cclip-tau tau, --robust-iters L). v_0 is the
  centre the previous round ended with; zeros before the first round, after a restart and after a
  resume: the centre is an estimate of the gradient, not model state, so it is not checkpointed and an
  elastic rollback leaves it as it is. For t = 1..L: a_k = fl32(min(1, tau / d_k(v_{t-1})) / W) (1/W
  at d_k = 0, 0 at +inf); b = fl32(1 - sum_k a_k); v_t = b v_{t-1} + sum_k a_k g_k. e = v_L, kept as
  the next round's centre.

Every combination is evaluated in fp32 per coordinate: it starts from fl(b v) (or 0) and adds fl(a_k
g_k) in source order. A wire with a_k == 0 is skipped (0 * inf would poison the sum). Weight sums and
distances are formed in double, in index order; the sum behind b runs over the rounded a_k. If all
a_k are 0 (every wire non-finite) e = 0 for geomed and the old centre for cclip, and the round is
counted in ``degenerate_rounds``; there is no fall-back to the mean.

Device: csrc/kernels/robust.hip, one launch for trimmed / median (a register sorting network per
lane), three for krum (the Gram matrix on MFMA, the selection in one workgroup, the selected sum);
csrc/kernels/robust_iter.hip for geomed / cclip: L + 1 fused passes over the wires (each forms the
new centre and the distances to it) and L one-workgroup weight steps, 2 L + 1 launches. No host
synchronisation: the counters stay in a device block that ``metrics`` reads once. CPU arena:
``combine_host``, the same definitions in torch.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops import kernels as K

KINDS = ("trimmed", "median", "krum", "geomed", "cclip")
ITERATIVE = ("geomed", "cclip")  # score the workers over the whole gradient, like krum


def min_sources(kind: str, trim: int = 1, byzantine: int = 1) -> int:
    """The fewest sources the rule is defined for."""
    return {"trimmed": 2 * trim + 1, "median": 1, "krum": 2 * byzantine + 3, "geomed": 3, "cclip": 3}[kind]


def check_sources(W: int, kind: str, trim: int = 1, byzantine: int = 1):
    need = min_sources(kind, trim, byzantine)
    if W < need:
        knob = {"trimmed": f"--trim {trim}", "krum": f"--byzantine {byzantine}"}.get(kind, "")
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


def iterate_host(X: torch.Tensor, kind: str, iters: int, tau: float, eps: float, centre=None):
    """geomed / cclip on the wires X [W, n] fp32 from the centre (fp32 [n]; None: zeros): the
    combination in fp32, weight sums and distances in double. Returns (v_L fp32 [n], the last a [W]
    float32, the distances [W] float64 behind it)."""
    W, n = X.shape
    Xd = X.double()
    v = torch.zeros(n, dtype=torch.float32) if centre is None else centre.clone()
    inf = float("inf")
    for _ in range(iters):
        d2 = ((Xd - v.double()) ** 2).sum(1).numpy()
        d = np.sqrt(np.where(np.isfinite(d2), d2, inf))
        with np.errstate(divide="ignore"):
            if kind == "geomed":
                w = np.where(np.isinf(d), 0.0, 1.0 / np.maximum(d, eps))
                S = 0.0
                for k in range(W):
                    S += float(w[k])
                a, b = (w / S if S > 0.0 else w * 0.0).astype(np.float32), np.float32(0.0)
            else:
                a = (np.where(np.isinf(d), 0.0, np.minimum(1.0, tau / d)) / W).astype(np.float32)
                S = 0.0
                for k in range(W):
                    S += float(a[k])
                b = np.float32(1.0 - S)
        s = v * float(b)
        for k in range(W):
            if a[k] != 0.0:
                s = s + X[k] * float(a[k])
        v = s
    return v, a, d


def combine_host(srcs: list, n: int, kind: str, trim: int = 1, byzantine: int = 1, c: float = 1.0, out=None,
                 iters: int = 3, tau: float = 0.0, eps: float = 1e-6, centre=None):
    """The estimate of the sources' first n elements times fl(c), in torch fp32 (the module
    docstring's definitions). Returns (out fp32 [n], the bool [W] selection of krum or None); for
    geomed / cclip the second value is (the final weights a [W] float32, the distances [W] float64
    behind them), and cclip's ``centre`` (fp32 [n], None: zeros) is advanced in place."""
    W = len(srcs)
    check_sources(W, kind, trim, byzantine)
    X = torch.stack([s[:n].to(torch.float32) for s in srcs])
    sel = None
    if kind in ITERATIVE:
        e, a, d = iterate_host(X, kind, iters, tau, eps, centre if kind == "cclip" else None)
        if kind == "cclip" and centre is not None:
            centre.copy_(e)
        sel = (a, d)
    elif kind == "krum":
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
        self.iters = int(getattr(cfg, "robust_iters", 3))
        self.tau, self.eps = float(getattr(cfg, "cclip_tau", 0.0)), float(getattr(cfg, "geomed_eps", 1e-6))
        self.n, self.device = n, torch.device(device)
        self.rounds = 0
        self._krum = self._host_selected = None
        if self.kind == "krum":
            if self.device.type == "cuda":
                self._krum = K.KrumState(n, self.device)
            else:
                self._host_selected = [0] * 32
        # geomed / cclip: the device scratch, state block and centre (ops/kernels.py RobustIterState), or on a CPU
        # arena the centre (cclip) and the same counters
        self._iter = self._host_centre = self._host_iter = None
        if self.kind in ITERATIVE:
            if self.device.type == "cuda":
                self._iter = K.RobustIterState(n, self.device, centre=self.kind == "cclip")
            else:
                self._host_centre = torch.zeros(n, dtype=torch.float32) if self.kind == "cclip" else None
                self._host_iter = {"degenerate_rounds": 0, "clipped": [0] * 32, "wsum": [0.0] * 32}

    def combine(self, srcs: list, out: torch.Tensor, weight: float, whole: bool) -> torch.Tensor:
        """out = e * c from the W unsummed dense wires (each holding the range in its first
        out.numel() elements), c = fl(1 / fl(weight)): the rule that follows multiplies its one
        already-summed source by ``weight``, so it applies the estimate e where weight is 1 / W, and
        any other weight (reference semantics) keeps its meaning as a scale on e."""
        W, n = len(srcs), out.numel()
        check_sources(W, self.kind, self.trim, self.byzantine)
        if (self.kind == "krum" or self.kind in ITERATIVE) and not whole:
            raise ValueError(f"--aggregate {self.kind} scores the workers over the whole gradient: a partial range of "
                             f"{n} of {self.n} elements cannot be combined (no bucketed or sharded updates)")
        c = float(np.float32(1.0) / np.float32(weight))
        srcs = [s if s.numel() == n else s[:n] for s in srcs]
        self.rounds += 1
        if self.device.type != "cuda":
            _, sel = combine_host(srcs, n, self.kind, self.trim, self.byzantine, c, out, self.iters, self.tau, self.eps,
                                  self._host_centre)
            if self.kind in ITERATIVE:
                a, d = sel
                h = self._host_iter
                h["degenerate_rounds"] += int(not a.any())
                for k in range(W):
                    h["wsum"][k] += float(a[k])
                    h["clipped"][k] += int(d[k] > self.tau)
            elif sel is not None:
                self._host_selected = [a + int(b) for a, b in zip(self._host_selected, sel.tolist() + [0] * (32 - W))]
        elif self.kind in ITERATIVE:
            st, L = self._iter, self.iters
            K.robust_iter_step(srcs, st, "init")
            for t in range(L):
                K.robust_iter_weights(st, W, self.kind, self.tau, self.eps, final=t == L - 1)
                if t < L - 1:
                    K.robust_iter_step(srcs, st, "mid")
            K.robust_iter_step(srcs, st, "last", agg=out, c=c)
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
        if self.kind in ITERATIVE:
            h = self._iter.read() if self._iter is not None else self._host_iter
            m["iters"], m["degenerate_rounds"] = self.iters, int(h["degenerate_rounds"])
            if self.kind == "geomed":
                # to 4 decimals: the device and the CPU arena sum their distances in different orders
                m["geomed_mean_weight_per_worker"] = [round(float(v) / max(1, self.rounds), 4)
                                                      for v in h["wsum"][:workers]]
            else:
                m["tau"] = self.tau
                m["cclip_clipped_per_worker"] = [int(v) for v in h["clipped"][:workers]]
        return m
