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
from ..ops import kernels as K
from ..utils import trace
from . import control as CP
from . import fetchq8, topk
from . import pushcodec as PC
from . import rules as R
from .core import APPLY, WAIT, ServerCore

_TRACE = os.environ.get("PSX_TRACE", "0") == "1"


def arena_sha256(arena: torch.Tensor) -> str:
    """sha256 (hex, first 32 digits) of an fp32 arena's bytes."""
    import hashlib

    return hashlib.sha256(arena.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()).hexdigest()[:32]


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
        # the one update rule of this server (parallel/rules.py): update_range runs it on every route
        self.rule = R.rule_of(cfg)
        # fp32 aggregation buffer: whole-arena rules stage every round's sum through it; otherwise
        # allocated when a path first needs it (in-process sync rounds, decoded payloads)
        self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device) if self.rule.whole else None
        # --optimizer lars / lamb: per-tensor ratios, in the device segment table + scratch
        # (ops/kernels.py LarsTable) or, on a CPU arena, the last update's list of the adapted tensors
        self._lars_tab = K.lars_table(layout, self.device) if self.rule.table and self.device.type == "cuda" else None
        self._lars_ratios = self._lamb_ratios = None
        self._ratios_applied = False
        # --optimizer adamw / lamb: both moments and the count of completed updates
        self.adam_m = torch.zeros_like(self.params) if self.rule.adam else None
        self.adam_v = torch.zeros_like(self.params) if self.rule.adam else None
        self.adam_t = 0
        # --clip-norm / --skip-nonfinite: no parameter state, only the counters: in the device state
        # block (ops/kernels.py GuardState), or in _guard_host on a CPU arena
        self._guard = cfg.grad_guard
        self._guard_state = self._guard_host = None
        self._guard_skip_logged = False
        if self._guard and self.device.type == "cuda":
            self._guard_state = K.GuardState(self.n, self.device)
        elif self._guard:
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
        # --fetch-codec q8delta (parallel/fetchq8.py): the fp32 shadow of what every worker holds and
        # the payload of the last encode, both allocated at the first fetch (fetch_delta).
        # shadow_valid goes false with every out-of-band change of the arena: the next fetch is a keyframe
        self.fetch_q8 = getattr(cfg, "fetch_codec", "") == "q8delta"
        self.shadow = self.fetch_payload = None
        self.shadow_valid = False
        self._fq_version = 0      # number of keyframes + encodes so far
        self._fq_step = None      # the global step the shadow stands at
        self._fq_key = False      # the last advance of the shadow was a keyframe
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
        (int32) / q8 or sign1 (uint8) payload. ``worker_id``: the pushing worker of an async push (delay
        compensation reads its backup)."""
        trace.mark("psx.apply")
        t0 = self._time_begin()
        if self._dc:
            self._apply_dc(grads, weight, worker_id)
            return self.finish_round_apply(self._time_end(t0))
        codec = self.codec_of(grads)
        if codec is PC.CODECS["topk"] and self.rule.scatters(self.cfg):
            # no optimizer state: scatter straight into the fp32 master parameters
            topk.decode_add(grads, self.params, -self.lr * weight, topk.topk_k(self.n, self.cfg.topk_ratio))
            self._wire_stale = True  # the bf16 image was not written by this update
            return self.finish_round_apply(self._time_end(t0))
        if codec.reducible:
            self.apply_range(grads[: self.n], weight, 0, self.n)
        else:  # a payload: decoded by the update entry
            self._apply_payloads([grads], weight)
        return self.finish_round_apply(self._time_end(t0))

    def _apply_payloads(self, payloads: list, weight: float):
        """The update from top-k, q8 or sign1 payloads (one codec per list), decoded and summed in
        fp32 in list order (update_range)."""
        self.update_range(payloads, weight, 0, self.n)

    def codec_of(self, t: torch.Tensor):
        """The push codec (parallel/pushcodec.py) of a pushed tensor, the configured one preferred."""
        return PC.of_payload(t, self.n, self.cfg.codec)

    def _dense_of(self, t: torch.Tensor, out: torch.Tensor | None = None, add: bool = False):
        """out = [out +] the dense fp32 gradient of a push of any codec (default: the aggregation buffer)."""
        return self.codec_of(t).decode(t, self.n, self._agg() if out is None else out, add, self.cfg.topk_ratio)

    # ------------------------------------------------------------------ the one update entry
    _IMG_OF_WIRE = object()

    def update_range(self, srcs: list, weight: float, lo: int, hi: int, img=_IMG_OF_WIRE, summed: bool = False):
        """The update of params[lo:hi] by this server's rule (parallel/rules.py); every route ends
        here. ``srcs``: fp16 / fp32 wires that each hold the gradient of exactly that range in their
        first hi - lo elements, summed in fp32 in list order, or the aggregation buffer itself (a
        decoded or accumulated sum); ``summed``: the one source already is the round's sum, taken
        as is. Payloads (whole range; their codec is told by parallel/pushcodec.py): q8 / sign1 are
        decoded inside the kernel by a rule that has such a device form (``device_payload``), every
        other case one after another into the aggregation buffer first. A rule that needs the whole arena
        refuses a partial range. ``img``: the bf16 image slice that receives the updated range, on
        the device in the same pass (default: the weight wire's, which an ``img`` of the caller's,
        and every host form, leaves stale). Several ranges of one round share the momentum 'first
        step' flag and the Adam update number: finish_round_apply closes the round."""
        rule = self.rule
        if rule.whole and (lo, hi) != (0, self.n):
            raise ValueError(rule.refusal.format(lo=lo, hi=hi, n=self.n))
        if hi <= lo:
            return
        on_device, own_img = self.device.type == "cuda", img is not self._IMG_OF_WIRE
        if on_device and not own_img:
            img = self.wire.img[lo:hi] if self.wire is not None else None
        codec = self.codec_of(srcs[0])
        if not codec.reducible:
            if on_device and codec.in_kernel is not None and rule.device_payload is not None:
                return rule.device_payload(self, codec, srcs, weight, img)
            for i, p in enumerate(srcs):
                self._dense_of(p, add=i > 0)
            srcs, summed = [self.agg], True
        if on_device:
            rule.device(self, srcs, weight, lo, hi, img, summed)
        elif rule.host(self, srcs, weight, lo, hi, summed) is False:
            return  # a skipped round: parameters and images are as they were
        elif own_img and img is not None:
            img.copy_(self.params[lo:hi])  # RNE, same bits as the kernels' f2bf
        if self.wire is not None and (own_img or not on_device):
            self._wire_stale = True  # the wire's image was not written by this update

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
        on every apply), then the usual tail. q8 / sign1 / top-k payloads are decoded into the aggregation
        buffer first. A worker without a valid backup (no fetch yet, or after a resume) is applied
        uncompensated and counted. Device: one launch of csrc/kernels/dcasgd.hip; CPU arena: the
        same formula in torch (equal to a tolerance, not bit for bit)."""
        cfg = self.cfg
        bak = self._dc_bak.get(worker_id) if worker_id in self._dc_valid else None
        if bak is None:
            self.dc_uncompensated += 1
        else:
            self.dc_compensated += 1
        if not self.codec_of(grads).reducible:
            grads = self._dense_of(grads)
        g = grads[: self.n]
        if bak is None and self._dc_ms is None:  # nothing of the DC form is left: the plain update
            return self.apply_range(g, weight, 0, self.n)
        if self.device.type == "cuda":
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

    def apply_range(self, g: torch.Tensor, weight: float, lo: int, hi: int):
        """The update restricted to params[lo:hi] (g holds exactly that slice): one bucket of a
        backward-overlapped sync round (parallel/overlap.py). Several ranges of one round share
        the same momentum 'first step' flag; finish_round_apply closes the round."""
        self.update_range([g], weight, lo, hi, summed=True)

    def apply_range_sources(self, srcs: list, weight: float, lo: int, hi: int):
        """apply_range of the fp32 sum of several wires' [lo:hi] (fixed list order): one bucket
        of an overlapped round whose wires were gathered (parallel/overlap.py)."""
        self.update_range([s[lo:hi] for s in srcs], weight, lo, hi)

    def lars_trust_ratios(self):
        """{min, median, max} of the last LARS update's trust ratios (rules.trust_ratios)."""
        return R.trust_ratios(self, R.LARS, self._lars_ratios)

    def lamb_trust_ratios(self):
        """{min, median, max} of the last LAMB update's ratios |w| / |u| (rules.trust_ratios)."""
        return R.trust_ratios(self, R.LAMB, self._lamb_ratios)

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
        if self.rule.adam:
            self.adam_t += 1
        if self._round_ev:
            self._ev_pending = self._ev_pending + [self._round_ev]
            self._round_ev = []
            dt = -1.0
        elif dt >= 0:
            self.update_time_source = "host clock (synchronous CPU apply)"
        self.core.on_applied(dt)
        return dt

    def _agg(self) -> torch.Tensor:
        if self.agg is None:
            self.agg = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        return self.agg

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

    # ------------------------------------------------------------------ delta fetch (--fetch-codec q8delta)
    def fetch_delta(self, keyframe: bool | None = None):
        """Bring the shadow up to the current global step and return (version, keyframe, payload).
        A keyframe sets shadow = arena (the caller ships the fp32 state; payload is not current);
        otherwise one encode of arena - shadow advances the shadow by what ``payload`` decodes to
        (fetchq8.encode_into). Once per update: further fetches of the same global step get the
        same answer. ``keyframe``: what a lockstep round expects (every rank derives it from the
        round number); None = decided here, by ``shadow_valid``."""
        n = self.arena.numel()
        if self.shadow is None:
            self.shadow = torch.empty_like(self.arena)
            self.fetch_payload = fetchq8.empty_payload(n, self.device)
        gs = self.core.global_step
        if keyframe is False and not self.shadow_valid:
            raise RuntimeError("q8delta: the arena changed outside the updates in mid-job; the workers of a "
                               "lockstep round cannot be told to take a keyframe")
        if keyframe or not self.shadow_valid:
            if not (self.shadow_valid and self._fq_key and self._fq_step == gs):
                self.shadow.copy_(self.arena)
                self._fq_version += 1
            self.shadow_valid, self._fq_key, self._fq_step = True, True, gs
        elif self._fq_step != gs:
            fetchq8.encode_into(self.arena, self.shadow, self.fetch_payload, n)
            self._fq_version += 1
            self._fq_key, self._fq_step = False, gs
        return self._fq_version, self._fq_key, self.fetch_payload

    def push_gradients(self, worker_id: int, grads: torch.Tensor, local_step: int, buffers=None) -> bool:
        """In-process push (single-process loopback runs). Sync: aggregate until the barrier
        completes, then apply the average. Async: staleness check + weighted apply.
        ``buffers`` (--bn-sync): the worker's BN running statistics, counted only when the core
        takes the push into the round (a duplicate / unknown / rejected push contributes nothing)."""
        self.bytes_pushed += self.codec_of(grads).wire_bytes(grads, self.n)
        res = self.core.on_push(worker_id, local_step)
        self.last_push = res
        if buffers is not None and (res.decision in (WAIT, APPLY) if self.cfg.mode == "sync" else res.accepted):
            self.push_buffers(worker_id, buffers)
        if self.cfg.mode == "sync":
            if self.cfg.sync_semantics == "reference":
                # reference: pending[worker_id] = grads (overwrites), average over the dict
                # entries when the push counter reaches total_workers (server.py:264-288)
                if res.decision in (WAIT, APPLY):
                    self._pending[worker_id] = self._dense_of(grads, torch.zeros(self.n, device=self.device))
                if res.apply:
                    self._dense_of(sum(self._pending.values()))
                    self._pending.clear()
                    self.apply(self.agg, res.weight)
                    self._commit_buffers()
                return True  # the reference always answers received=True in sync mode
            if res.apply and self._round_count == 0:
                # single-contribution round (W == 1): apply straight from the wire buffer — a dense
                # wire through the collective rounds' kernel (apply_sources with one source), so a
                # loopback round and a one-worker RCCL round (a shrunk sync job) give the same bits
                self._update_round([grads], res.weight)
                self._commit_buffers()
                return True
            if res.decision in (WAIT, APPLY):
                self._dense_of(grads, add=self._round_count != 0)
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
    def apply_round(self, srcs: list, members: list[int], local_steps: list[int],
                    buffers_sum: torch.Tensor | None = None, summed: bool = False) -> bool:
        """Bookkeeping + update for one sync round whose contributions reached rank 0 by a
        collective: ``srcs`` is the reduced sum (``summed``) or one gathered wire or payload per
        source (_update_round). True when the round's barrier completed and the update ran."""
        res = None
        for wid, ls in zip(members, local_steps):
            res = self.core.on_push(wid, ls)
        if summed:  # the reduce moved every member's wire
            self.bytes_pushed += len(members) * self.n * srcs[0].element_size()
        elif srcs:
            codec = self.codec_of(srcs[0])
            # a top-k gather holds a slot per rank, a dedicated server's empty one too: the members' count
            counted = srcs[: max(1, len(members))] if codec is PC.CODECS["topk"] else srcs
            self.bytes_pushed += sum(codec.wire_bytes(s, self.n) for s in counted)
        if res is None or not res.apply:
            return False
        self._update_round(list(srcs), res.weight, summed)
        if buffers_sum is not None:
            self.set_buffers_from_sum(buffers_sum, len(members))
        return True

    def _update_round(self, srcs: list, weight: float, summed: bool = False):
        """One timed update from a round's sources, closed by finish_round_apply. A reduced sum
        (``summed``) is taken as is; dense wires are summed in fp32 in list order inside the kernel
        (the reference's decompress + aggregate + apply, server.py:126-169, 232-237, without an
        fp16 running sum); payloads are decoded by the update entry (update_range)."""
        trace.mark("psx.apply")
        t0 = self._time_begin()
        self.update_range([srcs[0][: self.n]] if summed else srcs, weight, 0, self.n, summed=summed)
        self.finish_round_apply(self._time_end(t0))

    # the rounds by the name of how their sources arrived (channels, tests)
    def apply_reduced(self, summed, members, local_steps, buffers_sum=None) -> bool:
        return self.apply_round([summed], members, local_steps, buffers_sum, summed=True)

    def apply_sources(self, srcs, members, local_steps, buffers_sum=None) -> bool:
        return self.apply_round(srcs, members, local_steps, buffers_sum)

    apply_gathered = apply_payload_sources = apply_sources

    # ------------------------------------------------------------------ checkpoint
    def checkpoint(self, path: str | None = None) -> str:
        step = self.core.global_step
        path = path or ckpt.path_for(self.cfg.ckpt_dir, step)
        ckpt.save(path, self.layout, self.arena, self.counters, step, self.cfg.mode, self.total_workers,
                  self._base_lr, self.momentum_buf, self.cfg.to_json(), dc_meansquare=self._dc_ms,
                  adam=(self.adam_m, self.adam_v, self.adam_t) if self.rule.adam else None)
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
        self.shadow_valid = False  # q8delta: the next fetch is a keyframe
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
        if self.rule.adam:
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
        m.update(self.rule.metrics(self))
        if int(getattr(self.cfg, "warmup_steps", 0) or 0) > 0:
            m["warmup_steps"] = int(self.cfg.warmup_steps)
            m["effective_lr"] = float(self.lr)
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
        if self.fetch_q8:  # what every worker holds (their local_arena_sha256); None: nothing was fetched
            m["fetch_shadow_sha256"] = arena_sha256(self.shadow) if self.shadow_valid else None
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
        own = PC.CODECS[self.cfg.codec]
        slots = {w: own.slot(n, self.device, self.cfg.topk_ratio) for w in rank_of}
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
                        self.bytes_pushed += self.codec_of(grads).wire_bytes(grads, n)
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

