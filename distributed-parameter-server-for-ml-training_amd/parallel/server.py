"""The parameter server role (rank 0).

MI355X-native counterpart of the reference ParameterServerServicer
(reference: src/parameter_server/server.py:81-368):

* state lives in HBM: one fp32 arena holding the full state_dict (models/layout.py), an
  optional momentum buffer, a staging/aggregation buffer — no pickle, no param_lock: every
  update is one fused kernel (csrc/kernels/optim.hip) ordered on the server's HIP stream;
* decisions (registration ids, sync barrier, async staleness reject/weight, statistics) are
  made by the native core (csrc/runtime/ps_core.cpp, parallel/core.py);
* the reference RPC surface is kept for in-process use and naming parity:
  ``RegisterWorker``/``register_worker``, ``FetchParameters``/``fetch_parameters``,
  ``PushGradrients`` (sic, ps.proto:12) / ``PushGradients`` / ``push_gradients``,
  ``JobFinished``/``job_finished``;
* ``serve_async`` is the server event loop of the multi-process async mode: control
  requests arrive on the shared-memory mailbox, bulk tensors over RCCL point-to-point, and every
  fetch is served from a per-worker snapshot of the arena so in-flight sends never race the
  next update (the double-buffered arena of SURVEY.md §5.2).
"""
from __future__ import annotations

import os
import time

import torch

from ..utils import checkpoint as ckpt
from ..utils import metrics as M
from ..utils import trace
from . import control as CP
from . import q8, topk
from .core import APPLY, WAIT, ServerCore

_TRACE = os.environ.get("PSX_TRACE", "0") == "1"


def arena_sha256(arena: torch.Tensor) -> str:
    """sha256 (hex, first 32 digits) of an fp32 arena's bytes."""
    import hashlib

    return hashlib.sha256(arena.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()).hexdigest()[:32]


def _wire_bytes(grads: torch.Tensor, n: int) -> int:
    """Bytes one push moves: a q8 payload whole, otherwise the first n elements of the buffer."""
    if grads.dtype == torch.uint8:
        return grads.numel()
    return min(n, grads.numel()) * grads.element_size()


class ParameterServer:
    def __init__(self, cfg, layout, init_arena: torch.Tensor, counters: torch.Tensor | None = None, device="cpu",
                 total_workers: int | None = None, log=print):
        self.cfg = cfg
        self.layout = layout
        self.device = torch.device(device)
        self.total_workers = total_workers if total_workers is not None else cfg.workers
        self.lr = cfg.lr  # the configured base; reads give the open update's effective value (lr property)
        self.log = log if cfg.verbose else (lambda *a, **k: None)
        self.arena = init_arena.to(self.device, dtype=torch.float32).contiguous()
        self.counters = counters if counters is not None else torch.zeros(max(1, layout.num_counters), dtype=torch.int64)
        self.n = layout.param_numel
        self.params = self.arena[: self.n]
        self.momentum_buf = torch.zeros_like(self.params) if cfg.momentum else None
        self._mom_first = True
        self.agg = None  # fp32 aggregation buffer for in-process sync rounds
        # --optimizer lars: every whole-arena update goes through _lars_update (the LARS pair of
        # csrc/kernels/lars.hip, staged through agg); its only state is the momentum buffer
        self._lars = cfg.optimizer == "lars"
        self._lars_tab = None      # device segment table + scratch (ops/kernels.py LarsTable)
        self._lars_ratios = None   # CPU arena: the last update's trust ratios of the adapted tensors
        self._lars_applied = False
        if self._lars:
            self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            if self.device.type == "cuda":
                from ..ops import kernels as K

                self._lars_tab = K.lars_table(layout, self.device)
        # --optimizer adamw: element-wise, so every range of every path goes through _adamw_range
        # (csrc/kernels/adamw.hip); state: both moments and the count of completed updates
        self._adamw = cfg.optimizer == "adamw"
        self.adam_m = self.adam_v = None
        self.adam_t = 0
        # --optimizer lamb: the AdamW moments under the LARS table; every whole-arena update goes
        # through _lamb_update (the pair of csrc/kernels/lamb.hip, staged through agg)
        self._lamb = cfg.optimizer == "lamb"
        self._lamb_ratios = None   # CPU arena: the last update's ratios of the adapted tensors
        self._lamb_applied = False
        if self._lamb:
            self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            if self.device.type == "cuda":
                from ..ops import kernels as K

                self._lars_tab = K.lars_table(layout, self.device)
        if self._adamw or self._lamb:
            self.adam_m = torch.zeros_like(self.params)
            self.adam_v = torch.zeros_like(self.params)
        # --clip-norm / --skip-nonfinite: every whole-arena update goes through _guard_update (the
        # three launches of csrc/kernels/gguard.hip, staged through agg); no parameter state, only
        # the counters: in the device state block, or in _guard_host on a CPU arena
        self._guard = cfg.grad_guard
        self._guard_state = None   # device scratch + state block (ops/kernels.py GuardState)
        self._guard_host = None
        self._guard_skip_logged = False
        if self._guard:
            self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            if self.device.type == "cuda":
                from ..ops import kernels as K

                self._guard_state = K.GuardState(self.n, self.device)
            else:
                self._guard_host = {"rounds": 0, "clipped_rounds": 0, "skipped_rounds": 0, "norm_last": 0.0,
                                    "norm_max": 0.0, "norm_sum": 0.0}
        # --dc-lambda (async): delay compensation (csrc/kernels/dcasgd.hip). Every fetch leaves the
        # worker's backup of the fp32 parameters (note_fetch); the apply of a push from a worker
        # with a valid backup is g + lam * g * g * (w - bak) in place of g (_apply_dc).
        self._dc = cfg.dc_lambda > 0 and cfg.mode == "async"
        self._dc_bak = {}          # worker id -> fp32 [n] backup, allocated at the worker's first fetch
        self._dc_valid = set()     # worker ids whose backup holds their last fetch
        self._dc_ms = None         # --dc-adaptive: running mean square of the gradients, fp32 [n]
        self.dc_compensated = 0
        self.dc_uncompensated = 0
        if self._dc and cfg.dc_adaptive:
            self._dc_ms = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.wire = None  # WeightWire fetch payload kept current by the apply (enable_weight_wire)
        self._wire_stale = False
        self._pending = {}
        self.core = ServerCore(cfg.mode, self.total_workers, cfg.lr, cfg.staleness_bound, cfg.sync_semantics)
        self.start_time = time.time()
        self.bytes_pushed = 0
        self.bytes_fetched = 0
        self.images_processed = 0
        self.log(f"Initializing Parameter Server in {cfg.mode.upper()} mode on {self.device} "
                 f"({len(layout.entries)} state_dict tensors, {self.n:,} trainable params)")
        if cfg.resume:
            self.resume(cfg.resume)

    # ------------------------------------------------------------------ learning rate (--warmup-steps)
    @property
    def lr(self) -> float:
        """The learning rate of the open update, number k = completed updates + 1 (the count
        finish_round_apply advances and resume restores): lr * min(1, k / warmup_steps), in
        double; the configured lr with --warmup-steps 0. Every update path reads it at call time."""
        n = int(getattr(self.cfg, "warmup_steps", 0) or 0)
        if n <= 0:
            return self._base_lr
        return self._base_lr * min(1.0, (self.core.global_step + 1) / n)

    @lr.setter
    def lr(self, value: float):
        self._base_lr = float(value)

    # ------------------------------------------------------------------ numerics
    def apply(self, grads: torch.Tensor, weight: float, worker_id: int | None = None):
        """p <- p - lr * (weight * g [+ wd p]) [momentum]; grads are fp16 wire, fp32, or a top-k
        (int32) / q8 (uint8) payload. ``worker_id``: the pushing worker of an async push (delay
        compensation reads its backup)."""
        trace.mark("psx.apply")
        t0 = self._time_begin()
        if self._dc:
            self._apply_dc(grads, weight, worker_id)
            return self.finish_round_apply(self._time_end(t0))
        if grads.dtype == torch.int32:  # top-k payload (parallel/topk.py)
            if not self.cfg.momentum and not self.cfg.weight_decay and not self._lars and not self._guard \
                    and not self._adamw and not self._lamb:
                # no optimizer state: scatter straight into the fp32 master parameters
                topk.decode_add(grads, self.params, -self.lr * weight, self._kcap)
                self._wire_stale = True  # the bf16 image was not written by this update
                return self.finish_round_apply(self._time_end(t0))
            grads = self._dense_of(grads)
        if grads.dtype == torch.uint8:  # q8 payload (parallel/q8.py): decoded inside the update
            self._apply_q8([grads], weight)
        else:
            self.apply_range(grads[: self.n], weight, 0, self.n)
        return self.finish_round_apply(self._time_end(t0))

    def _apply_q8(self, payloads: list, weight: float):
        """The update from q8 payloads, decoded and summed in fp32 in list order: one fused
        launch on the device (the weight image, when enabled, written in the same pass); the
        torch decode into the aggregation buffer on a CPU arena. LARS: decoded into the
        aggregation buffer on either, then the dense entry of the LARS pair; the gradient guard
        likewise (its dense entry), AdamW (the one-source fp32 form of its kernel) and LAMB (its
        dense entry)."""
        if self.device.type == "cuda" and not self._lars and not self._guard and not self._adamw and not self._lamb:
            from ..ops import kernels as K

            img = self.wire.img[: self.n] if self.wire is not None else None
            K.q8_apply_multi(self.params, payloads, self.lr, gscale=weight, momentum=self.cfg.momentum,
                             wd=self.cfg.weight_decay, buf=self.momentum_buf, first=self._mom_first, n=self.n, img=img)
            return
        for i, p in enumerate(payloads):
            self._dense_of(p, add=i > 0)
        self.apply_range(self.agg, weight, 0, self.n)

    # ------------------------------------------------------------------ delay compensation (--dc-lambda)
    def note_fetch(self, worker_id: int, dst: torch.Tensor | None = None) -> int:
        """Worker ``worker_id`` fetches the current state: the core's bookkeeping and, with delay
        compensation on, the worker's backup of the fp32 parameters, taken in stream order with
        the applies. ``dst`` (optional, the worker's fp32 arena) also receives the arena — on the
        device from the same read as the backup (kernels.dc_fetch_copy). Returns the global step."""
        gs = self.core.on_fetch(worker_id)
        if not self._dc:
            if dst is not None:
                dst.copy_(self.arena)
            return gs
        bak = self._dc_bak.get(worker_id)
        if bak is None:
            bak = self._dc_bak[worker_id] = torch.empty(self.n, dtype=torch.float32, device=self.device)
        fused = (self.device.type == "cuda" and (dst is None or (
            dst.dtype == torch.float32 and dst.device == self.arena.device and dst.is_contiguous()
            and dst.numel() == self.arena.numel())))
        if fused:
            from ..ops import kernels as K

            K.dc_fetch_copy(self.arena, dst, bak, self.n)
        else:
            bak.copy_(self.params)
            if dst is not None:
                dst.copy_(self.arena)
        self._dc_valid.add(worker_id)
        return gs

    def _apply_dc(self, grads: torch.Tensor, weight: float, worker_id):
        """The delay-compensated update of one async push: g~ = g + lam * g * g * (w - bak), lam =
        dc_lambda or dc_lambda / sqrt(ms + dc_eps) (adaptive; ms = decay * ms + (1 - decay) * g * g
        on every apply), then the usual tail. q8 / top-k payloads are decoded into the aggregation
        buffer first. A worker without a valid backup (no fetch yet, or after a resume) is applied
        uncompensated and counted. Device: one launch of csrc/kernels/dcasgd.hip; CPU arena: the
        same formula in torch (equal to a tolerance, not bit for bit)."""
        cfg = self.cfg
        bak = self._dc_bak.get(worker_id) if worker_id in self._dc_valid else None
        if bak is None:
            self.dc_uncompensated += 1
        else:
            self.dc_compensated += 1
        if grads.dtype in (torch.int32, torch.uint8):
            grads = self._dense_of(grads)
        g = grads[: self.n]
        if bak is None and self._dc_ms is None:  # nothing of the DC form is left: the plain update
            return self.apply_range(g, weight, 0, self.n)
        if self.device.type == "cuda":
            from ..ops import kernels as K

            img = self.wire.img[: self.n] if self.wire is not None else None
            K.dc_apply(self.params, g, bak, self.lr, cfg.dc_lambda, ms=self._dc_ms, decay=cfg.dc_decay,
                       eps=cfg.dc_eps, gscale=weight, momentum=cfg.momentum, wd=cfg.weight_decay,
                       buf=self.momentum_buf, first=self._mom_first, n=self.n, img=img)
            return
        g = g.to(torch.float32)
        lam = cfg.dc_lambda
        if self._dc_ms is not None:
            self._dc_ms.mul_(cfg.dc_decay).add_((1.0 - cfg.dc_decay) * g * g)
            lam = cfg.dc_lambda / torch.sqrt(self._dc_ms + cfg.dc_eps)
        if bak is not None:
            g = g + lam * g * g * (self.params - bak)
        self.apply_range(g, weight, 0, self.n)

    # ------------------------------------------------------------------ update timing
    # The reference times the apply itself (server.py:128,140-141) into average_update_time_seconds.
    # Here the apply is an asynchronous kernel, so its time is the DEVICE time between two timing
    # events recorded around it on the update stream; the pair is read back lazily (when a later
    # apply starts, or at final_metrics) and fed to the core. A round applied in several ranges
    # (gradient buckets of an overlapped round) sums its ranges. CPU arenas use the host clock.
    # Applies captured into a HIP graph cannot be bracketed: they leave no sample.
    _round_ev: list = []
    _ev_pending: list = []
    update_time_source = "none"

    def _time_begin(self):
        if self.device.type != "cuda":
            return time.perf_counter()
        if torch.cuda.is_current_stream_capturing():
            return None
        self._drain_update_times()
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _time_end(self, tok):
        """Closes one timed range; returns the host seconds (CPU) or -1 (device: deferred)."""
        if tok is None:
            return -1.0
        if isinstance(tok, float):
            return time.perf_counter() - tok
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        self._round_ev = self._round_ev + [(tok, end)]
        return -1.0

    def _drain_update_times(self, block: bool = False):
        keep = []
        for pairs in self._ev_pending:
            if block or all(e.query() for _, e in pairs):
                s = sum(b.elapsed_time(e) for b, e in pairs) * 1e-3  # elapsed_time waits for e
                self.core.record_update_time(s)
                self.update_time_source = "device events around the apply kernels"
            else:
                keep.append(pairs)
        self._ev_pending = keep

    @property
    def _kcap(self) -> int:
        return topk.topk_k(self.n, self.cfg.topk_ratio)

    def _dense_of(self, payload: torch.Tensor, out: torch.Tensor | None = None, add: bool = False):
        """Top-k / q8 payload -> dense fp32 gradient (into the aggregation buffer by default)."""
        if out is None:
            if self.agg is None:
                self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            out = self.agg
        if payload.dtype == torch.uint8:
            return q8.decode(payload, self.n, out=out, add=add)
        if not add:
            out.zero_()
        return topk.decode_add(payload, out, 1.0, self._kcap)

    def apply_range(self, g: torch.Tensor, weight: float, lo: int, hi: int):
        """The update restricted to params[lo:hi] (g holds exactly that slice): one bucket of a
        backward-overlapped sync round (parallel/overlap.py). Several ranges of one round share
        the same momentum 'first step' flag; finish_round_apply closes the round."""
        if self._lars:
            self._lars_whole(lo, hi)
            return self._lars_update([g], weight)
        if self._lamb:
            self._lamb_whole(lo, hi)
            return self._lamb_update([g], weight)
        if self._guard:
            self._guard_whole(lo, hi)
            return self._guard_update([g], weight)
        self._sgd_range(g, weight, lo, hi)

    def _sgd_range(self, g: torch.Tensor, weight: float, lo: int, hi: int):
        """apply_range's plain SGD form (no LARS, no guard routing); AdamW's under --optimizer adamw."""
        if self._adamw:
            return self._adamw_range([g], weight, lo, hi)
        p = self.params[lo:hi]
        buf = self.momentum_buf[lo:hi] if self.momentum_buf is not None else None
        if self.device.type == "cuda":
            from ..ops import kernels as K

            img = self.wire.img[lo:hi] if self.wire is not None else None  # fetch image, same pass
            K.sgd_apply(p, g, self.lr, gscale=weight, momentum=self.cfg.momentum, wd=self.cfg.weight_decay, buf=buf,
                        first=self._mom_first, n=hi - lo, img=img)
            return
        if self.wire is not None:
            self._wire_stale = True
        d = g.to(torch.float32) * weight
        if self.cfg.weight_decay:
            d = d + self.cfg.weight_decay * p
        if buf is not None:
            if self._mom_first:
                buf.copy_(d)
            else:
                buf.mul_(self.cfg.momentum).add_(d)
            d = buf
        p.sub_(self.lr * d)

    def apply_range_sources(self, srcs: list, weight: float, lo: int, hi: int):
        """apply_range of the fp32 sum of several wires' [lo:hi] (fixed list order): one bucket
        of an overlapped round whose wires were gathered (parallel/overlap.py)."""
        if self._lars:
            self._lars_whole(lo, hi)
            return self._lars_update(list(srcs), weight)
        if self._lamb:
            self._lamb_whole(lo, hi)
            return self._lamb_update(list(srcs), weight)
        if self._guard:
            self._guard_whole(lo, hi)
            return self._guard_update(list(srcs), weight)
        if self._adamw:
            return self._adamw_range([s[lo:hi] for s in srcs], weight, lo, hi)
        if self.device.type == "cuda":
            from ..ops import kernels as K

            buf = self.momentum_buf[lo:hi] if self.momentum_buf is not None else None
            img = self.wire.img[lo:hi] if self.wire is not None else None
            K.sgd_apply_multi(self.params[lo:hi], [s[lo:hi] for s in srcs], self.lr, gscale=weight,
                              momentum=self.cfg.momentum, wd=self.cfg.weight_decay, buf=buf, first=self._mom_first,
                              n=hi - lo, img=img)
            return
        agg = torch.zeros(hi - lo, dtype=torch.float32, device=self.device)
        for s in srcs:  # fixed order, fp32 accumulation
            agg.add_(s[lo:hi].to(torch.float32))
        self.apply_range(agg, weight, lo, hi)

    # ------------------------------------------------------------------ AdamW (--optimizer adamw)
    _IMG_OF_WIRE = object()

    def _adamw_range(self, srcs: list, weight: float, lo: int, hi: int, img=_IMG_OF_WIRE):
        """The AdamW update of params[lo:hi] from sources that each hold exactly that slice (fp16 /
        fp32 wires summed in fp32 in list order, or one dense fp32 sum), update number adam_t + 1:
        g = weight * s; m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g g;
        p = p (1 - lr wd) - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
        Element-wise: any range is legal, and every range of one round shares t
        (finish_round_apply closes the round). ``img``: the bf16 image slice to write (default: the
        weight wire's). Device: one launch of csrc/kernels/adamw.hip; CPU arena: the same formula in
        torch fp32 from the same eight fp32 scalars (equal to a tolerance, not bit for bit)."""
        import numpy as np

        from ..ops import kernels as K

        cfg = self.cfg
        n, t = hi - lo, self.adam_t + 1
        if n <= 0:
            return
        p, m, v = self.params[lo:hi], self.adam_m[lo:hi], self.adam_v[lo:hi]
        hp = dict(beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_eps, wd=cfg.weight_decay)
        if self.device.type == "cuda":
            if img is self._IMG_OF_WIRE:
                img = self.wire.img[lo:hi] if self.wire is not None else None
            K.adamw_apply_multi(p, [s[:n] for s in srcs], m, v, self.lr, t, gscale=weight, n=n, img=img, **hp)
            return
        try:
            step_size, b1, omb1, b2, omb2, rbc2, eps, decay = K.adamw_scalars(self.lr, t, **hp)
        except (OSError, RuntimeError, AttributeError):  # the kernel library is not loaded here
            step_size, b1, omb1, b2, omb2, rbc2, eps, decay = K.adamw_scalars_host(self.lr, t, **hp)
        if self.wire is not None:
            self._wire_stale = True
        s = torch.zeros(n, dtype=torch.float32, device=self.device)
        for x in srcs:  # fixed order, fp32 accumulation
            s = s + x[:n].to(torch.float32)
        # plain element-wise fp32 ops only (no fused alpha forms): a range gives the whole round's bits
        g = s * float(np.float32(weight))
        m.copy_(m * b1 + g * omb1)
        v.copy_(v * b2 + (g * g) * omb2)
        den = v.sqrt() * rbc2 + eps
        p.copy_(p * decay - (m / den) * step_size)

    # ------------------------------------------------------------------ LARS (--optimizer lars)
    def _lars_whole(self, lo: int, hi: int):
        if (lo, hi) != (0, self.n):
            raise ValueError(f"--optimizer lars needs every tensor's norm before its first element moves: a partial "
                             f"range [{lo}, {hi}) of {self.n} cannot be applied (no bucketed or sharded updates)")

    def _lars_update(self, srcs: list, weight: float):
        """The whole-arena LARS update from dense wires (fp16 / fp32, summed in fp32 in list
        order) or from the aggregation buffer itself (a decoded or accumulated sum):
        d = lambda_t * (weight * s + wd * w) for tensors with ndim > 1, lambda_t = trust * |w| /
        (weight * |s| + wd * |w| + eps) (1 when a norm is 0); d = weight * s for 1-D tensors;
        then the momentum form of apply_range. Device: the two launches of csrc/kernels/lars.hip;
        CPU arena: the same formula in torch, tensor by tensor (equal to a tolerance, not bit for
        bit: the reduction orders differ)."""
        cfg = self.cfg
        self._lars_applied = True
        staged = len(srcs) == 1 and srcs[0].dtype == torch.float32 and srcs[0].data_ptr() == self.agg.data_ptr()
        if self.device.type == "cuda":
            from ..ops import kernels as K

            kw = dict(lr=self.lr, gscale=weight, momentum=cfg.momentum, wd=cfg.weight_decay, trust=cfg.lars_trust,
                      eps=cfg.lars_eps, buf=self.momentum_buf, first=self._mom_first, n=self.n,
                      img=self.wire.img[: self.n] if self.wire is not None else None)
            if staged:
                K.lars_apply(self.params, self.agg, self._lars_tab, **kw)
            else:
                K.lars_apply_multi(self.params, [s[: self.n] for s in srcs], self.agg, self._lars_tab, **kw)
            return
        if not staged:
            self.agg.zero_()
            for s in srcs:  # fixed order, fp32 accumulation
                self.agg.add_(s[: self.n].to(torch.float32))
        if self.wire is not None:
            self._wire_stale = True
        ratios = []
        for e in self.layout.entries.values():
            if e.region != "param" or not e.numel:
                continue
            w = self.params[e.offset:e.offset + e.numel]
            d = self.agg[e.offset:e.offset + e.numel] * weight
            if len(e.shape) > 1:
                wn, gn = float(w.double().norm()), float(d.double().norm())
                lam = cfg.lars_trust * wn / (gn + cfg.weight_decay * wn + cfg.lars_eps) if wn > 0 and gn > 0 else 1.0
                ratios.append(lam)
                if cfg.weight_decay:
                    d = d + cfg.weight_decay * w
                d = d * lam
            if self.momentum_buf is not None:
                buf = self.momentum_buf[e.offset:e.offset + e.numel]
                if self._mom_first:
                    buf.copy_(d)
                else:
                    buf.mul_(cfg.momentum).add_(d)
                d = buf
            w.sub_(self.lr * d)
        self._lars_ratios = ratios

    def lars_trust_ratios(self):
        """{min, median, max} of the last update's trust ratios over the adapted tensors (read
        from the device ratio table here, not per round); None before the first update."""
        if not self._lars_applied:
            return None
        if self._lars_tab is not None:
            r = self._lars_tab.ratios.cpu()[torch.tensor(self._lars_tab.adapt)]
        else:
            r = torch.tensor(self._lars_ratios)
        if not r.numel():
            return None
        return {"min": float(r.min()), "median": float(r.median()), "max": float(r.max())}

    # ------------------------------------------------------------------ LAMB (--optimizer lamb)
    def _lamb_whole(self, lo: int, hi: int):
        if (lo, hi) != (0, self.n):
            raise ValueError(f"--optimizer lamb needs every tensor's norm before its first element moves: a partial "
                             f"range [{lo}, {hi}) of {self.n} cannot be applied (no bucketed or sharded updates)")

    def _lamb_update(self, srcs: list, weight: float):
        """The whole-arena LAMB update (You et al. 2020), number adam_t + 1, from dense wires (fp16
        / fp32, summed in fp32 in list order) or from the aggregation buffer itself (a decoded or
        accumulated sum): g = weight * s; m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g g;
        r = m / (1 - beta1^t) / (sqrt(v) / sqrt(1 - beta2^t) + eps); tensors with ndim > 1: u = r +
        wd * w, phi = |w| / |u| (1 when a norm is 0); 1-D tensors: u = r, phi = 1; w -= lr * phi * u.
        No clamp on |w|, no global gradient normalisation. Device: the two launches of
        csrc/kernels/lamb.hip (the aggregation buffer ends holding u); CPU arena: the same formula
        in torch from the same fp32 scalars, tensor by tensor (equal to a tolerance, not bit for
        bit: the reduction orders differ)."""
        import numpy as np

        from ..ops import kernels as K

        cfg = self.cfg
        self._lamb_applied = True
        t = self.adam_t + 1
        hp = dict(beta1=cfg.adam_beta1, beta2=cfg.adam_beta2, eps=cfg.adam_eps)
        staged = len(srcs) == 1 and srcs[0].dtype == torch.float32 and srcs[0].data_ptr() == self.agg.data_ptr()
        if self.device.type == "cuda":
            kw = dict(lr=self.lr, t=t, gscale=weight, wd=cfg.weight_decay, n=self.n,
                      img=self.wire.img[: self.n] if self.wire is not None else None, **hp)
            if staged:
                K.lamb_apply(self.params, self.agg, self.adam_m, self.adam_v, self._lars_tab, **kw)
            else:
                K.lamb_apply_multi(self.params, [s[: self.n] for s in srcs], self.agg, self.adam_m, self.adam_v,
                                   self._lars_tab, **kw)
            return
        if not staged:
            self.agg.zero_()
            for s in srcs:  # fixed order, fp32 accumulation
                self.agg.add_(s[: self.n].to(torch.float32))
        if self.wire is not None:
            self._wire_stale = True
        try:
            bc1, b1, omb1, b2, omb2, rbc2, eps, _ = K.lamb_scalars(t, **hp)
        except (OSError, RuntimeError, AttributeError):  # the kernel library is not loaded here
            bc1, b1, omb1, b2, omb2, rbc2, eps, _ = K.lamb_scalars_host(t, **hp)
        lr, wd = float(np.float32(self.lr)), float(np.float32(cfg.weight_decay))
        g = self.agg * float(np.float32(weight))
        self.adam_m.copy_(self.adam_m * b1 + g * omb1)
        self.adam_v.copy_(self.adam_v * b2 + (g * g) * omb2)
        r = (self.adam_m / (self.adam_v.sqrt() * rbc2 + eps)) * bc1
        ratios = []
        for e in self.layout.entries.values():
            if e.region != "param" or not e.numel:
                continue
            w = self.params[e.offset:e.offset + e.numel]
            u = r[e.offset:e.offset + e.numel]
            phi = 1.0
            if len(e.shape) > 1:
                u = u + wd * w
                wn, un = float(w.double().norm()), float(u.double().norm())
                phi = float(np.float32(wn / un)) if wn > 0 and un > 0 else 1.0
                ratios.append(phi)
            w.sub_(float(np.float32(lr * phi)) * u)
        self._lamb_ratios = ratios

    def lamb_trust_ratios(self):
        """{min, median, max} of the last update's ratios |w| / |u| over the adapted tensors (read
        from the device ratio table here, not per round); None before the first update."""
        if not self._lamb_applied:
            return None
        if self._lars_tab is not None:
            r = self._lars_tab.ratios.cpu()[torch.tensor(self._lars_tab.adapt)]
        else:
            r = torch.tensor(self._lamb_ratios)
        if not r.numel():
            return None
        return {"min": float(r.min()), "median": float(r.median()), "max": float(r.max())}

    # ------------------------------------------------------------------ gradient guard (--clip-norm, --skip-nonfinite)
    def _guard_whole(self, lo: int, hi: int):
        if (lo, hi) != (0, self.n):
            raise ValueError(f"--clip-norm / --skip-nonfinite need the whole gradient's norm before the first parameter "
                             f"moves: a partial range [{lo}, {hi}) of {self.n} cannot be applied (no bucketed or "
                             f"sharded updates)")

    def _guard_update(self, srcs: list, weight: float):
        """The whole-arena guarded update from dense wires (fp16 / fp32, summed in fp32 in list
        order) or from the aggregation buffer itself (a decoded or accumulated sum):
        S = sum s^2, norm = weight * sqrt(S); S not finite: the round is skipped (parameters,
        momentum buffer and fetch image untouched; it still counts as a round, and consumes the
        momentum 'first step' flag: the buffer starts as zeros, so momentum * 0 + d of the next
        round has the value the first-step form would have given); else coef = min(1, clip_norm /
        (norm + 1e-6)) (1 without --clip-norm), rounded to fp32, and apply_range's update with
        weight * coef (one fp32 multiply): weight decay is added after the scaling, not clipped.
        Device: the three launches of csrc/kernels/gguard.hip, no host synchronisation; CPU arena:
        the same formula in torch (equal to a tolerance, not bit for bit: the reduction orders
        differ)."""
        cfg = self.cfg
        staged = len(srcs) == 1 and srcs[0].dtype == torch.float32 and srcs[0].data_ptr() == self.agg.data_ptr()
        if self.device.type == "cuda":
            from ..ops import kernels as K

            kw = dict(lr=self.lr, gscale=weight, momentum=cfg.momentum, wd=cfg.weight_decay, clip_norm=cfg.clip_norm,
                      buf=self.momentum_buf, first=self._mom_first, n=self.n,
                      img=self.wire.img[: self.n] if self.wire is not None else None)
            if staged:
                K.guard_apply(self.params, self.agg, self._guard_state, **kw)
            else:
                K.guard_apply_multi(self.params, [s[: self.n] for s in srcs], self.agg, self._guard_state, **kw)
            return
        import math

        import numpy as np

        if not staged:
            self.agg.zero_()
            for s in srcs:  # fixed order, fp32 accumulation
                self.agg.add_(s[: self.n].to(torch.float32))
        S = float(self.agg.double().square().sum())
        h = self._guard_host
        h["rounds"] += 1
        if not math.isfinite(S):
            h["skipped_rounds"] += 1
            h["norm_last"] = float("nan") if S != S else float("inf")
            return
        norm = float(np.float32(weight)) * math.sqrt(S)
        coef = np.float32(min(1.0, cfg.clip_norm / (norm + 1e-6))) if cfg.clip_norm > 0 else np.float32(1.0)
        h["clipped_rounds"] += int(coef < 1.0)
        h["norm_last"] = norm
        h["norm_max"] = max(h["norm_max"], norm)
        h["norm_sum"] += norm
        self._sgd_range(self.agg, float(np.float32(weight) * coef), 0, self.n)

    def guard_counters(self):
        """The guard's running counters (read from the device state block here, not per round);
        None with the guard off. Not rolled back by an elastic shrink: a round that was applied and
        then rolled back stays counted."""
        if not self._guard:
            return None
        h = self._guard_state.read() if self._guard_state is not None else self._guard_host
        if h["skipped_rounds"] and not self._guard_skip_logged:
            self._guard_skip_logged = True
            self.log(f"[GradientGuard] {h['skipped_rounds']} of {h['rounds']} updates so far skipped: "
                     f"non-finite gradient sum")
        fin = h["rounds"] - h["skipped_rounds"]
        return {"clip_norm": float(self.cfg.clip_norm), "rounds": int(h["rounds"]),
                "clipped_rounds": int(h["clipped_rounds"]), "skipped_rounds": int(h["skipped_rounds"]),
                "norm_last": float(h["norm_last"]), "norm_max": float(h["norm_max"]),
                "norm_mean": float(h["norm_sum"]) / fin if fin else None}

    def finish_round_apply(self, dt: float = -1.0):
        """Closes one update (global_step + 1). ``dt`` >= 0: its host-measured time (CPU arena);
        else the device ranges timed since the last close (deferred), or none (graph capture)."""
        self._mom_first = False
        if self._adamw or self._lamb:
            self.adam_t += 1
        if self._round_ev:
            self._ev_pending = self._ev_pending + [self._round_ev]
            self._round_ev = []
            dt = -1.0
        elif dt >= 0:
            self.update_time_source = "host clock (synchronous CPU apply)"
        self.core.on_applied(dt)
        return dt

    def _accumulate(self, grads: torch.Tensor, first: bool):
        if self.agg is None:
            self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        if grads.dtype in (torch.int32, torch.uint8):
            self._dense_of(grads, self.agg, add=not first)
            return
        if first:
            self.agg.copy_(grads[: self.n])
        else:
            self.agg.add_(grads[: self.n].to(torch.float32))

    # ------------------------------------------------------------------ RPC surface
    def register_worker(self, worker_name: str = "worker-node", requested_id: int = -1):
        wid = self.core.register(worker_name, requested_id)
        self.log(f"[RegisterWorker] Worker {wid} from {worker_name} registered")
        self.log(f"Active workers: {self.core.num_active()}/{self.total_workers}")
        return wid, self.total_workers

    def fetch_parameters(self, worker_id: int):
        gs = self.note_fetch(worker_id)
        self.bytes_fetched += self.arena.numel() * 4
        return self.arena, gs

    # ------------------------------------------------------------------ weight-image fetch path
    def enable_weight_wire(self):
        """Keep a WeightWire (parallel/codec.py) of the current state: the apply kernel writes
        its bf16 image in the same pass as the fp32 update; the fp32 remainder is gathered per
        fetch. Fetches then ship/copy exactly that one buffer."""
        from .codec import WeightWire

        if self.wire is None:
            self.wire = WeightWire(self.layout, self.device)
        self.wire.publish_full(self.arena)
        self._wire_stale = False
        return self.wire

    def wire_for_fetch(self, publish_small: bool = True):
        """The WeightWire holding the current state (fp32 remainder refreshed unless the only
        reader gathers it from the arena itself; the image was written by the apply, or is
        rebuilt here after an out-of-band update)."""
        if self._wire_stale:
            self.wire.publish_full(self.arena)
            self._wire_stale = False
        elif publish_small:
            self.wire.publish_small(self.arena)
        return self.wire

    def fetch_wire(self, worker_id: int, publish_small: bool = True):
        gs = self.note_fetch(worker_id)
        w = self.wire_for_fetch(publish_small)
        self.bytes_fetched += w.nbytes
        return w, gs

    def push_gradients(self, worker_id: int, grads: torch.Tensor, local_step: int, buffers=None) -> bool:
        """In-process push (single-process loopback runs). Sync: aggregate until the barrier
        completes, then apply the average. Async: staleness check + weighted apply.
        ``buffers`` (--bn-sync): the worker's BN running statistics, counted only when the core
        takes the push into the round (a duplicate / unknown / rejected push contributes nothing)."""
        self.bytes_pushed += _wire_bytes(grads, self.n)
        res = self.core.on_push(worker_id, local_step)
        self.last_push = res
        if buffers is not None and (res.decision in (WAIT, APPLY) if self.cfg.mode == "sync" else res.accepted):
            self.push_buffers(worker_id, buffers)
        if self.cfg.mode == "sync":
            if self.cfg.sync_semantics == "reference":
                # reference: pending[worker_id] = grads (overwrites), average over the dict
                # entries when the push counter reaches total_workers (server.py:264-288)
                if res.decision in (WAIT, APPLY):
                    self._pending[worker_id] = (self._dense_of(grads, torch.zeros(self.n, device=self.device))
                                                if grads.dtype in (torch.int32, torch.uint8)
                                                else grads[: self.n].to(torch.float32).clone())
                if res.apply:
                    self._accumulate(sum(self._pending.values()), True)
                    self._pending.clear()
                    self.apply(self.agg, res.weight)
                    self._commit_buffers()
                return True  # the reference always answers received=True in sync mode
            if res.apply and self._round_count == 0:
                # single-contribution round (W == 1): apply straight from the wire buffer — a dense
                # wire through the collective rounds' kernel (apply_sources with one source), so a
                # loopback round and a one-worker RCCL round (a shrunk sync job) give the same bits
                if grads.dtype == torch.int32:  # decoded into the dense buffer first, as apply_gathered
                    self._dense_of(grads)
                    self.apply(self.agg, res.weight)
                elif grads.dtype == torch.uint8:  # one-source q8_apply_multi, as apply_q8_sources
                    self.apply(grads, res.weight)
                else:
                    trace.mark("psx.apply")
                    t0 = self._time_begin()
                    self.apply_range_sources([grads], res.weight, 0, self.n)
                    self.finish_round_apply(self._time_end(t0))
                self._commit_buffers()
                return True
            if res.decision in (WAIT, APPLY):
                self._accumulate(grads, self._round_count == 0)
                self._round_count += 1
            if res.apply:
                self.apply(self.agg, res.weight)
                self._commit_buffers()
                self._round_count = 0
            return res.accepted
        if res.apply:
            self.apply(grads, res.weight, worker_id)
        return res.accepted

    _round_count = 0
    _pending: dict = {}
    last_push = None
    _buf_acc = None
    _buf_n = 0

    # ------------------------------------------------------------------ BN running stats (--bn-sync)
    def push_buffers(self, worker_id: int, bufs: torch.Tensor):
        """Worker BN running statistics (float buffer region of its local arena). Sync: averaged
        over the round (committed with the round's update); async: blended with weight 1/W."""
        if self.layout.buffer_numel == 0:
            return
        region = self.arena[self.n:]
        if self.cfg.mode == "sync":
            if self._buf_acc is None:
                self._buf_acc = torch.zeros_like(region)
            self._buf_acc.add_(bufs.to(region.device))
            self._buf_n += 1
        else:
            w = 1.0 / max(1, self.total_workers)
            region.mul_(1.0 - w).add_(bufs.to(region.device), alpha=w)

    def _commit_buffers(self):
        if self._buf_n:
            self.arena[self.n:].copy_(self._buf_acc / self._buf_n)
            self._buf_acc.zero_()
            self._buf_n = 0

    def set_buffers_from_sum(self, summed: torch.Tensor, count: int):
        self.arena[self.n:].copy_(summed / max(1, count))

    def job_finished(self, worker_id: int, emit: bool = True) -> str:
        """Reference server.py:306-318: when the last active worker finishes, print the final
        statistics (runners that append job-level fields pass emit=False and emit once)."""
        self.log(f"[JobFinished] Worker {worker_id} completed")
        if self.core.job_finished(worker_id) and emit:
            self.final_metrics(emit=True)
        return "Acknowledged"

    # reference RPC names (ps.proto:4-19, including the PushGradrients typo)
    RegisterWorker = register_worker
    FetchParameters = fetch_parameters
    PushGradients = push_gradients
    PushGradrients = push_gradients
    JobFinished = job_finished

    # ------------------------------------------------------------------ sync (collective) path
    def apply_reduced(self, summed: torch.Tensor, members: list[int], local_steps: list[int],
                      buffers_sum: torch.Tensor | None = None) -> bool:
        """Bookkeeping + update for one sync round whose gradient sum arrived by RCCL reduce."""
        res = None
        for wid, ls in zip(members, local_steps):
            res = self.core.on_push(wid, ls)
        self.bytes_pushed += len(members) * self.n * summed.element_size()
        if res is not None and res.apply:
            self.apply(summed, res.weight)
            if buffers_sum is not None:
                self.set_buffers_from_sum(buffers_sum, len(members))
            return True
        return False

    def apply_sources(self, srcs: list, members: list[int], local_steps: list[int],
                      buffers_sum: torch.Tensor | None = None) -> bool:
        """Sync round whose W dense wires were gathered to rank 0 (one per contributing worker):
        decoded and summed in fp32 in list order inside the update (kernels.sgd_apply_multi),
        then p -= lr * sum / W — the reference's decompress + aggregate + apply
        (server.py:126-169, 232-237) without an fp16 running sum."""
        res = None
        for wid, ls in zip(members, local_steps):
            res = self.core.on_push(wid, ls)
        self.bytes_pushed += sum(s[: self.n].numel() * s.element_size() for s in srcs)
        if res is None or not res.apply:
            return False
        trace.mark("psx.apply")
        t0 = self._time_begin()
        if self._lars:
            self._lars_update(list(srcs), res.weight)
        elif self._lamb:
            self._lamb_update(list(srcs), res.weight)
        elif self._guard:
            self._guard_update(list(srcs), res.weight)
        elif self._adamw:
            self._adamw_range([s[: self.n] for s in srcs], res.weight, 0, self.n)
        elif self.device.type == "cuda":
            from ..ops import kernels as K

            img = self.wire.img[: self.n] if self.wire is not None else None
            K.sgd_apply_multi(self.params, [s[: self.n] for s in srcs], self.lr, gscale=res.weight,
                              momentum=self.cfg.momentum, wd=self.cfg.weight_decay, buf=self.momentum_buf,
                              first=self._mom_first, n=self.n, img=img)
        else:
            if self.agg is None:
                self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            self.agg.zero_()
            for s in srcs:  # fixed order, fp32 accumulation
                self.agg.add_(s[: self.n].to(torch.float32))
            self.apply_range(self.agg, res.weight, 0, self.n)
        self.finish_round_apply(self._time_end(t0))
        if buffers_sum is not None:
            self.set_buffers_from_sum(buffers_sum, len(members))
        return True

    def apply_gathered(self, payloads: list, members: list[int], local_steps: list[int],
                       buffers_sum: torch.Tensor | None = None) -> bool:
        """Sync round with top-k payloads gathered to rank 0: decode all into one dense fp32
        sum, then the usual averaged apply."""
        res = None
        for wid, ls in zip(members, local_steps):
            res = self.core.on_push(wid, ls)
        self.bytes_pushed += sum(p.numel() * 4 for p in payloads[: max(1, len(members))])
        if res is not None and res.apply:
            for i, p in enumerate(payloads):
                self._dense_of(p, add=i > 0)
            self.apply(self.agg, res.weight)
            if buffers_sum is not None:
                self.set_buffers_from_sum(buffers_sum, len(members))
            return True
        return False

    def apply_q8_sources(self, payloads: list, members: list[int], local_steps: list[int],
                         buffers_sum: torch.Tensor | None = None) -> bool:
        """Sync round whose W q8 payloads were gathered to rank 0 (one per contributing worker):
        the bookkeeping of apply_sources, then one launch that decodes and sums them in fp32 in
        list order inside the update (kernels.q8_apply_multi) — no dense staging buffer."""
        res = None
        for wid, ls in zip(members, local_steps):
            res = self.core.on_push(wid, ls)
        self.bytes_pushed += sum(p.numel() for p in payloads)
        if res is None or not res.apply:
            return False
        trace.mark("psx.apply")
        t0 = self._time_begin()
        self._apply_q8(list(payloads), res.weight)
        self.finish_round_apply(self._time_end(t0))
        if buffers_sum is not None:
            self.set_buffers_from_sum(buffers_sum, len(members))
        return True

    # ------------------------------------------------------------------ checkpoint
    def checkpoint(self, path: str | None = None) -> str:
        step = self.core.global_step
        path = path or ckpt.path_for(self.cfg.ckpt_dir, step)
        ckpt.save(path, self.layout, self.arena, self.counters, step, self.cfg.mode, self.total_workers,
                  self._base_lr, self.momentum_buf, self.cfg.to_json(), dc_meansquare=self._dc_ms,
                  adam=(self.adam_m, self.adam_v, self.adam_t) if self._adamw or self._lamb else None)
        self.log(f"[Checkpoint] global step {step} -> {path}")
        return path

    def maybe_checkpoint(self):
        if self.cfg.ckpt_every and self.core.global_step % self.cfg.ckpt_every == 0 and self.core.global_step:
            return self.checkpoint()
        return None

    def resume(self, path: str):
        if path == "latest":
            path = ckpt.latest(self.cfg.ckpt_dir)
            if path is None:
                self.log("[Resume] no checkpoint found; starting fresh")
                return
        arena, counters, step, mom, obj = ckpt.restore(path, self.layout)
        self.arena.copy_(arena.to(self.device))
        self._wire_stale = True
        self.counters = counters
        self.core.global_step = step
        if mom is not None and self.momentum_buf is not None:
            self.momentum_buf.copy_(mom.to(self.device))
            self._mom_first = False
        # delay compensation: the mean square travels with the checkpoint (absent in older ones: it
        # stays zero); the backups do not, so every worker is uncompensated until its next fetch
        self._dc_valid.clear()
        ms = obj.get("server_optimizer_state", {}).get("dc_meansquare")
        if ms is not None and self._dc_ms is not None:
            self._dc_ms.copy_(ms.to(self.device))
        # AdamW / LAMB: both moments and the update count (absent, e.g. an SGD server's checkpoint:
        # zero moments, the next update is t = 1)
        if self._adamw or self._lamb:
            st = obj.get("server_optimizer_state", {})
            if st.get("adam_m") is not None and st.get("adam_v") is not None:
                self.adam_m.copy_(st["adam_m"].to(self.device))
                self.adam_v.copy_(st["adam_v"].to(self.device))
                self.adam_t = int(st.get("adam_step", 0))
            else:
                self.adam_m.zero_()
                self.adam_v.zero_()
                self.adam_t = 0
        self.log(f"[Resume] restored global step {step} from {path}")

    # ------------------------------------------------------------------ metrics
    def final_metrics(self, emit: bool = False, extra: dict | None = None) -> dict:
        if self._ev_pending:
            self._drain_update_times(block=True)
        m = self.core.metrics()
        m["update_time_source"] = self.update_time_source
        m["optimizer"] = self.cfg.optimizer
        if self._lars:
            m["lars_trust_ratio"] = self.lars_trust_ratios()
        if self._adamw:
            m["adamw"] = {"beta1": float(self.cfg.adam_beta1), "beta2": float(self.cfg.adam_beta2),
                          "eps": float(self.cfg.adam_eps), "steps": int(self.adam_t)}
        if self._lamb:
            m["lamb"] = {"beta1": float(self.cfg.adam_beta1), "beta2": float(self.cfg.adam_beta2),
                         "eps": float(self.cfg.adam_eps), "steps": int(self.adam_t)}
            m["lamb_trust_ratio"] = self.lamb_trust_ratios()
        if int(getattr(self.cfg, "warmup_steps", 0) or 0) > 0:
            m["warmup_steps"] = int(self.cfg.warmup_steps)
            m["effective_lr"] = float(self.lr)
        if self._guard:
            m["gradient_guard"] = self.guard_counters()
        if self._dc:
            m["delay_compensation"] = {"lambda": float(self.cfg.dc_lambda), "adaptive": bool(self.cfg.dc_adaptive),
                                       "compensated_pushes": int(self.dc_compensated),
                                       "uncompensated_pushes": int(self.dc_uncompensated)}
        m["bytes_pushed"] = int(self.bytes_pushed)
        m["bytes_fetched"] = int(self.bytes_fetched)
        if self.images_processed:
            m["images_processed"] = int(self.images_processed)
        # fingerprints of the final master state: sum |p| (order-independent, for tolerance checks)
        # and the sha256 of the fp32 arena bytes (bit-equality checks across runs / modes)
        m["final_param_checksum"] = float(self.arena.double().abs().sum())
        m["final_param_sha256"] = arena_sha256(self.arena)
        if extra:
            m.update(extra)
        if emit:
            self.log(f"\n{'=' * 50}\nPARAMETER SERVER FINAL STATISTICS\n{'=' * 50}")
            self.log(f"Mode: {m['mode'].upper()}  workers: {m['total_workers']}  global steps: "
                     f"{m['global_steps_completed']}  updates/s: {m['updates_per_second']}")
            M.emit(m, self.cfg.log_dir, rank=0)
            self.log("--- End Server Metrics ---")
        return m

    # ------------------------------------------------------------------ async event loop
    def serve_async(self, transport, mbox, rank_of: dict, stop_when_done: bool = True, local_queue=None,
                    poll: float = 0.0005, expected: int | None = None):
        """Multi-process async server loop (runs on rank 0, in its own thread when rank 0 also
        trains). rank_of: worker_id -> transport rank of the *remote* workers. ``local_queue``
        (optional) delivers requests of the co-located worker as (kind, worker_id, grads,
        local_step, event, box). The loop ends once ``expected`` workers finished or died."""
        expected = expected if expected is not None else len(rank_of) + (1 if local_queue is not None else 0)
        finished = set()
        n = self.n
        if self.cfg.codec == "topk":
            words = topk.payload_words(self._kcap)
            slots = {w: torch.empty(words, dtype=torch.int32, device=self.device) for w in rank_of}
        elif self.cfg.codec == "q8":
            slots = {w: torch.empty(q8.payload_bytes(n), dtype=torch.uint8, device=self.device) for w in rank_of}
        else:
            wire_dtype = torch.float16 if self.cfg.codec == "fp16" else torch.float32
            slots = {w: torch.empty(n, dtype=wire_dtype, device=self.device) for w in rank_of}
        # one fetch snapshot per worker (codec wire buffers): an in-flight send never races the
        # next update of the arena
        from .codec import FetchCodec

        snaps = {w: FetchCodec(self.layout, self.cfg.fetch_codec, self.device) for w in rank_of}
        bufslots = {}
        pending_recv = []   # (wid, local_step, work, buffers_work)
        pending_send = {}   # wid -> [works]
        last_to = time.monotonic()
        while True:
            msg = mbox.recv(timeout=poll)
            if msg is not None and _TRACE:
                print(f"[psx-server] {msg} pending_recv={[p[0] for p in pending_recv]}", flush=True)
            if msg is not None:
                t, wid = msg.type, msg.a
                if t == CP.HELLO:
                    got, total = self.register_worker(f"rank{msg.src}", msg.a)
                    mbox.reply(msg.src, CP.Msg(CP.R_REGISTERED, 0, got, total))
                elif t == CP.FETCH:
                    gs = self.note_fetch(wid)
                    for prev in pending_send.pop(wid, []):
                        prev.wait()
                    pending_send[wid] = [transport.isend(b, rank_of[wid]) for b in snaps[wid].pack(self.arena)]
                    self.bytes_fetched += snaps[wid].nbytes
                    mbox.reply(rank_of[wid], CP.Msg(CP.R_FETCHED, 0, wid, 0, gs))
                elif t == CP.PUSH:
                    work = transport.irecv(slots[wid], rank_of[wid])
                    bwork = None
                    if msg.b:  # BN running statistics follow the gradients (--bn-sync)
                        if wid not in bufslots:
                            bufslots[wid] = torch.empty(self.layout.buffer_numel, dtype=torch.float32,
                                                        device=self.device)
                        bwork = transport.irecv(bufslots[wid], rank_of[wid])
                    pending_recv.append((wid, msg.c, work, bwork))
                elif t == CP.DONE:
                    finished.add(wid)
                    self.core.job_finished(wid)
                    mbox.reply(rank_of[wid], CP.Msg(CP.R_ACK, 0, wid))
                    self.log(f"[JobFinished] Worker {wid} completed")
                elif t == CP.HEARTBEAT:
                    self.core.heartbeat(wid)
                elif t == CP.STOP:
                    break
            # complete arrived pushes in arrival order
            keep = []
            for wid, ls, work, bwork in pending_recv:
                if transport.completed(work):  # each work is waited exactly once (gloo!)
                    if bwork is not None:
                        transport.completed(bwork) or bwork.wait()
                    res = self.core.on_push(wid, ls)
                    self.bytes_pushed += slots[wid].numel() * slots[wid].element_size()
                    if res.apply:
                        self.apply(slots[wid], res.weight, wid)
                        if bwork is not None:
                            self.push_buffers(wid, bufslots[wid])
                        self.maybe_checkpoint()
                    mbox.reply(rank_of[wid], CP.Msg(CP.R_PUSHED, 0, wid, int(res.accepted), self.core.global_step,
                                                    res.staleness))
                else:
                    keep.append((wid, ls, work, bwork))
            pending_recv = keep
            stop = False
            if local_queue is not None:
                while True:
                    try:
                        kind, wid, grads, ls, ev, box = local_queue.get_nowait()
                    except Exception:
                        break
                    if kind == "push":
                        res = self.core.on_push(wid, ls)
                        self.bytes_pushed += _wire_bytes(grads, n)
                        if res.apply:
                            self.apply(grads, res.weight, wid)
                            if box.get("bufs") is not None:
                                self.push_buffers(wid, box["bufs"])
                            self.maybe_checkpoint()
                        box["res"] = res
                        box["global_step"] = self.core.global_step
                    else:  # "done"
                        self.log(f"[JobFinished] Worker {wid} completed")
                        self.core.job_finished(wid)
                        finished.add(wid)
                    ev.set()
            now = time.monotonic()
            if self.cfg.heartbeat_timeout and now - last_to > 1.0:
                last_to = now
                for w in self.core.check_timeouts(self.cfg.heartbeat_timeout):
                    self.log(f"[Failure] worker {w} missed heartbeats for {self.cfg.heartbeat_timeout}s; marked dead")
                    finished.add(w)
            if stop_when_done and len(finished) >= expected and not pending_recv:
                break
        for works in pending_send.values():
            for w in works:
                w.wait()

