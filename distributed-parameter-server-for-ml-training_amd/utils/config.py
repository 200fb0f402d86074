"""Configuration: CLI flags + environment defaults + optional JSON file.

Keeps every flag and environment variable of the reference with the same defaults
(reference: src/parameter_server/server.py:405-433 and src/workers/worker.py:455-482):

  server  --mode {sync,async}  env SERVER_MODE             default sync
          --workers N (1..32)  env TOTAL_WORKERS_EXPECTED  default 4
          --lr 0.1, --port (env SERVER_PORT, 8000), --staleness-bound 5 (now actually wired)
  worker  --server (env PARAMETER_SERVER_ADDRESS, localhost:8000), --worker-name,
          --epochs 3, --batch-size 128, --lr 0.1, --sync-steps 1

and adds the MI355X-native knobs: --gpus/--nproc, --codec {none,fp16,q8,sign1,topk},
--topk-ratio,
--dtype, --momentum/--weight-decay (server optimizer, default 0 = reference parity),
--optimizer {sgd,lars,adamw,lamb} with --lars-trust/--lars-eps and --adam-beta1/--adam-beta2/--adam-eps,
--warmup-steps (linear lr warmup of the server update),
--dc-lambda/--dc-adaptive (async delay compensation), --clip-norm/--skip-nonfinite (global-norm clipping, non-finite guard), --model,
--synthetic, --ckpt-every/--resume, --sync-semantics {barrier,reference}, --topology.
Precedence: explicit CLI flag > JSON config file (--config) > environment > default.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
from dataclasses import dataclass, field


def _env(name, default, cast=str):
    v = os.environ.get(name)
    return cast(v) if v not in (None, "") else default


def _push_codecs() -> dict:
    """The table of push codecs, keyed by the --codec values (parallel/pushcodec.py)."""
    from ..parallel.pushcodec import CODECS

    return CODECS


@dataclass
class PSConfig:
    # --- reference server flags
    mode: str = "sync"
    workers: int = 4
    lr: float = 0.1
    port: int = 8000
    staleness_bound: int = 5
    # --- reference worker flags
    server: str = "localhost:8000"
    worker_name: str = "worker-node"
    epochs: int = 3
    batch_size: int = 128
    sync_steps: int = 1
    # --- MI355X-native extensions
    accumulate: bool = False       # --sync-steps K: push the mean gradient of the K batches of a window
    #                                instead of the reference's first batch only (K-1 discarded)
    model: str = "resnet18"
    num_classes: int | None = None
    gpus: int = 1                  # processes / GPUs on this node (1 = server+worker co-located)
    topology: str = "colocated"    # colocated: rank 0 = PS + worker 0; dedicated: rank 0 = PS only;
    #                                sharded: every rank = worker + 1/world of the PS (parallel/sharded.py)
    codec: str = "fp16"            # none (fp32 wire) | fp16 (reference) | q8 (block-scaled int8) | sign1 (1 bit) | topk
    topk_ratio: float = 0.01
    # compute dtype of the HIP engine: fp32 = the reference's training precision (worker.py:333-348;
    # exact-f32 MFMA), bf16 = the fast path (bf16 operands, fp32 accumulation and master weights)
    dtype: str = "fp32"
    momentum: float = 0.0          # server optimizer (0 = reference plain SGD, server.py:133)
    weight_decay: float = 0.0
    # server optimizer: sgd (the flat update above) | lars (layer-wise adaptive: every tensor with
    # ndim > 1 gets the trust ratio lars_trust * |w| / (|g| + wd |w| + lars_eps) and the weight
    # decay, 1-D tensors neither; csrc/kernels/lars.hip). Runs on the Python server's whole-arena
    # updates only: no native loops, graph round, bucketed overlap or sharded server.
    optimizer: str = "sgd"
    lars_trust: float = 0.001
    lars_eps: float = 1e-8
    # adamw (csrc/kernels/adamw.hip): Adam moments with bias correction and the decoupled weight
    # decay of torch.optim.AdamW, p <- p (1 - lr wd) - lr mhat / (sqrt(vhat) + adam_eps); weight_decay
    # applies to every trainable element, 0 = plain Adam. Element-wise, so unlike lars it also runs
    # on bucketed overlapped rounds and on the sharded server; momentum must be 0 (beta1 is the
    # momentum). Python server only: no native loops, graph round or elastic shrink.
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    # lamb (csrc/kernels/lamb.hip, You et al. 2020): the adamw moments (adam_beta1 / adam_beta2 /
    # adam_eps) with a per-tensor ratio |w| / |u| on the update u = mhat / (sqrt(vhat) + adam_eps) +
    # wd w of every tensor with ndim > 1; 1-D tensors take ratio 1 and no weight decay (the lars
    # convention). No clamp on |w|, no global gradient normalisation. Scope as lars: the Python
    # server's whole-arena updates only; momentum must be 0.
    # warmup_steps N > 0: update number k (1-based) runs with lr * min(1, k / N); 0 = constant lr.
    # Python server only: the native loops and the graph round hold a fixed lr.
    warmup_steps: int = 0
    # async delay compensation (DC-ASGD, csrc/kernels/dcasgd.hip): the server keeps the parameters
    # each worker last fetched (bak) and applies g + lam * g * g * (w - bak) in place of g.
    # dc_lambda 0 = off; dc_adaptive: lam = dc_lambda / sqrt(ms + dc_eps) with ms the running mean
    # square of the gradients (decay dc_decay). Async mode, SGD server, unsharded.
    dc_lambda: float = 0.0
    dc_adaptive: bool = False
    dc_decay: float = 0.95
    dc_eps: float = 1e-7
    # gradient guard (csrc/kernels/gguard.hip): clip_norm C > 0 scales a round whose global gradient
    # norm (of the weighted fp32 sum the server applies) exceeds C by C / (norm + 1e-6), torch's
    # clip_grad_norm_ form, weight decay not clipped; skip_nonfinite drops a round whose sum holds
    # inf / NaN instead of poisoning the arena. clip_norm > 0 implies skip_nonfinite. SGD server,
    # whole-arena updates only: no bucketed overlap, graph round, sharded server, native async loop.
    clip_norm: float = 0.0
    skip_nonfinite: bool = False
    sync_semantics: str = "barrier"  # barrier (wait-for-N) | reference (count-triggered)
    # The reference server never updates BN running statistics and every fetch overwrites the
    # workers' copies (server.py:96,131-133 + worker.py:252), so evaluation runs on near-initial
    # statistics. bn_sync=True makes workers push their running stats with each gradient push;
    # the server averages them (sync) or blends them 1/W (async). Default off = reference parity.
    bn_sync: bool = False
    deterministic: bool | None = None  # exact fixed-point BN reductions, bit-reproducible steps; None:
    # PSX_DETERMINISTIC (default 1 = on; engine)
    # fetch payload: "bf16conv" = conv weights as bf16 (exactly the bits the bf16 engine consumes)
    # + fp32 for everything else (half the bytes); "fp32" = the reference's full fp32 state;
    # "auto" = fp32 for --dtype fp32, bf16conv for --dtype bf16; "q8delta" = after one fp32 keyframe,
    # the block-scaled int8 of what changed since the workers' copy (1.016 bytes per element, error
    # feedback; parallel/fetchq8.py). Sync mode, rank-0 server, serial rounds, either --dtype.
    fetch_codec: str = "auto"
    # sync rounds stream gradient buckets during the backward pass (parallel/overlap.py). None =
    # auto: on with >= 2 ranks (the gather / apply / broadcast of the first buckets hides under
    # the rest of the backward), off at N=1, where there is no transfer to hide and the
    # per-bucket graphs cost ~0.2 ms/step (profiles/README.md). resolve_overlap() decides.
    overlap: object = None
    bucket_mb: float = 4.0         # bucket target size in MiB of fp16 wire gradient
    synthetic: bool = True
    synthetic_kind: str = "proto"  # proto: prototype + noise (learnable); hard: low contrast + 20% label noise
    data_dir: str = ""
    train_samples: int = 50000
    test_samples: int = 10000
    eval_every: int = 1            # epochs between evaluations (0 = never)
    eval_workers: str = "all"      # all: every worker evaluates (reference worker.py:393-394); first: worker 0 only
    max_steps: int = 0             # stop after this many local steps (0 = full epochs)
    ckpt_every: int = 0
    ckpt_dir: str = "checkpoints"
    resume: str = ""
    seed: int = 0
    heartbeat_timeout: float = 60.0
    log_dir: str = ""
    use_graph: bool = True
    # "kill_worker:2@5" (worker 2 raises at its step 5) | "hang_worker:2@5[:secs]" (stalls, forever or secs)
    # | "crash_in_push:2@5" (async: worker 2's process dies inside its step-5 push, after the PUSH request)
    fault_inject: str = ""
    transfer_timeout: float = 300.0  # async native loop: drop a worker whose transfer is in flight longer (0: off)
    stall_timeout: float = 0.0       # async native loop: drop a worker silent (no request) that long (0: off)
    round_timeout: float = 300.0   # sync liveness guard: abort + exit 3 when no round completes (0: off)
    # sync, dedicated topology: what a lost worker does to the job. shrink: the survivors rebuild
    # the communicator in-process and go on (parallel/elastic.py); restart: abort, exit 3, the
    # launcher restarts the group from the last checkpoint
    on_worker_loss: str = "shrink"
    recovery_grace: float = 0.0    # s the server waits for survivors to check in (0: --round-timeout)
    verbose: int = 1
    extra: dict = field(default_factory=dict)

    def validate(self):
        if self.mode not in ("sync", "async"):
            raise ValueError(f"--mode must be sync or async, got {self.mode!r}")
        if not (1 <= self.workers <= 32):  # reference server.py:424-426
            raise ValueError("Number of workers must be between 1 and 32")
        if self.eval_workers not in ("all", "first"):
            raise ValueError("--eval-workers must be all or first")
        if self.codec not in _push_codecs():
            raise ValueError(f"--codec must be none, fp16, q8, sign1 or topk, got {self.codec!r}")
        if self.topology not in ("colocated", "dedicated", "sharded"):
            raise ValueError(f"--topology must be colocated, dedicated or sharded, got {self.topology!r}")
        if self.optimizer not in ("sgd", "lars", "adamw", "lamb"):
            raise ValueError(f"--optimizer must be sgd, lars, adamw or lamb, got {self.optimizer!r}")
        if self.optimizer in ("adamw", "lamb"):
            opt = f"--optimizer {self.optimizer}"
            if not (0.0 <= self.adam_beta1 < 1.0) or not (0.0 <= self.adam_beta2 < 1.0):
                raise ValueError(f"{opt}: --adam-beta1 and --adam-beta2 must be in [0, 1)")
            if not self.adam_eps > 0.0:
                raise ValueError(f"{opt}: --adam-eps must be > 0")
            if self.momentum:
                raise ValueError(f"{opt}: --adam-beta1 is the momentum, --momentum must be 0")
        if int(self.warmup_steps) < 0:
            raise ValueError("--warmup-steps must be >= 0")
        if self.optimizer == "lars" and (not (self.lars_trust > 0.0) or self.lars_eps < 0.0):
            raise ValueError("--optimizer lars: --lars-trust must be > 0 and --lars-eps >= 0")
        if self.dc_lambda < 0.0:
            raise ValueError("--dc-lambda must be >= 0")
        if self.dc_adaptive and not self.dc_lambda > 0.0:
            raise ValueError("--dc-adaptive scales --dc-lambda: give --dc-lambda > 0")
        if not (0.0 <= self.dc_decay < 1.0):
            raise ValueError("--dc-decay must be in [0, 1)")
        if self.dc_lambda > 0.0:
            if self.mode != "async":  # every sync push has staleness 0: nothing to compensate
                raise ValueError("--dc-lambda compensates gradient staleness: --mode async only")
            if self.optimizer != "sgd":
                raise ValueError(f"--dc-lambda runs on the SGD server update: not with --optimizer {self.optimizer}")
        if not self.clip_norm >= 0.0:
            raise ValueError("--clip-norm must be >= 0")
        if self.clip_norm > 0.0:
            self.skip_nonfinite = True
        if self.grad_guard:
            if self.optimizer != "sgd":
                raise ValueError(f"--clip-norm / --skip-nonfinite run on the SGD server update: not with --optimizer "
                                 f"{self.optimizer}")
            if self.dc_lambda > 0.0:
                raise ValueError("--clip-norm / --skip-nonfinite run on the SGD server update: not with --dc-lambda")
        if self.whole_arena_update:
            # a shard boundary or a gradient bucket may split a tensor (lars, lamb); no shard sees the
            # whole gradient, and a bucket is applied before the others have arrived (the guard)
            who, one_server, at_once = (f"--optimizer {self.optimizer}", "needs whole tensors on one server",
                                        "updates the whole arena at once")
            if self.grad_guard:
                who, one_server, at_once = ("--clip-norm / --skip-nonfinite", "need the whole gradient's norm on one "
                                            "server", "need the whole gradient's norm before the first parameter moves")
            if self.topology == "sharded":
                raise ValueError(f"{who} {one_server}: not with --topology sharded")
            if self.overlap is True:
                raise ValueError(f"{who} {at_once}: not with --overlap")
        if self.topology == "sharded":  # parallel/sharded.py scope
            if self.mode != "sync" or self.codec not in ("fp16", "none") or self.bn_sync or self.ckpt_every \
                    or self.resume or max(1, self.sync_steps) != 1 or self.overlap is True:
                raise ValueError("--topology sharded: sync mode, dense fp16/fp32 gradients, one push per batch, "
                                 "no --bn-sync / --overlap / checkpoints")
        if self.sync_semantics not in ("barrier", "reference"):
            raise ValueError("--sync-semantics must be barrier or reference")
        if self.staleness_bound < 0:
            raise ValueError("--staleness-bound must be >= 0")
        if self.on_worker_loss not in ("shrink", "restart"):
            raise ValueError("--on-worker-loss must be shrink or restart")
        if self.transfer_timeout < 0 or self.stall_timeout < 0:
            raise ValueError("--transfer-timeout / --stall-timeout must be >= 0")
        if self.dtype not in ("fp32", "bf16"):
            raise ValueError(f"--dtype must be fp32 or bf16, got {self.dtype!r}")
        if self.fetch_codec == "auto":
            self.fetch_codec = "fp32" if self.dtype == "fp32" else "bf16conv"
        if self.fetch_codec not in ("bf16conv", "fp32", "q8delta"):
            raise ValueError("--fetch-codec must be bf16conv, fp32 or q8delta")
        if self.fetch_codec == "q8delta":  # parallel/fetchq8.py scope
            if self.mode != "sync":
                raise ValueError("--fetch-codec q8delta keeps one shadow of the workers' copy, which only lockstep "
                                 "rounds keep equal on every worker: --mode sync only (async would need a shadow "
                                 "per worker)")
            if self.topology == "sharded":
                raise ValueError("--fetch-codec q8delta encodes the whole arena on a rank-0 server: not with "
                                 "--topology sharded (its fetch is an all-gather of per-rank ranges)")
            if self.overlap is True:
                raise ValueError("--fetch-codec q8delta encodes the arena once it is final: not with --overlap "
                                 "(a bucketed round broadcasts each bucket before the others are applied)")
        if self.dtype == "fp32" and self.fetch_codec == "bf16conv":
            raise ValueError("--fetch-codec bf16conv ships bf16 conv weights, which only the bf16 engine consumes: "
                             "add --dtype bf16 (the default since round 2 is --dtype fp32, the reference's "
                             "precision, whose fetch payload is the fp32 state)")
        if self.bucket_mb <= 0:
            raise ValueError("--bucket-mb must be > 0")
        if self.synthetic_kind not in ("proto", "hard"):
            raise ValueError("--synthetic-kind must be proto or hard")
        if not (0.0 < self.topk_ratio <= 1.0):
            raise ValueError("--topk-ratio must be in (0, 1]")
        if self.fault_inject.startswith("crash_in_push") and self.mode != "async":
            # only the async native channel can die between its PUSH request and the transfer
            raise ValueError("--fault-inject crash_in_push applies to --mode async (native event loop) only")
        return self

    def resolve_overlap(self, world: int) -> bool:
        """--overlap / --no-overlap, or auto: bucketed rounds when there are peers to exchange
        with and the round qualifies (sync, one push per batch, dense wire, rank-0 server). The
        error-feedback codecs (q8, sign1, topk) encode the whole gradient at once, and a whole-arena update
        (whole_arena_update) cannot start before the last bucket: no bucketed rounds. --optimizer
        adamw is element-wise and stays eligible. --fetch-codec q8delta encodes the final arena of a
        round, which a bucketed round broadcasts piecewise before it exists: no bucketed rounds."""
        if self.overlap is None:
            self.overlap = (world > 1 and self.mode == "sync" and max(1, self.sync_steps) == 1
                            and self.dense_wire and self.topology != "sharded" and not self.whole_arena_update
                            and self.fetch_codec != "q8delta")
        return bool(self.overlap)

    @property
    def whole_arena_update(self) -> bool:
        """The server update needs a norm over the whole arena (every tensor's for --optimizer lars
        / lamb, the whole gradient's for the gradient guard) before the first element moves: no
        --topology sharded, no --overlap."""
        return self.optimizer in ("lars", "lamb") or self.grad_guard

    @property
    def grad_guard(self) -> bool:
        """The gradient guard is on: --clip-norm > 0 or --skip-nonfinite."""
        return self.clip_norm > 0.0 or bool(self.skip_nonfinite)

    @property
    def dense_wire(self) -> bool:
        """The push is the dense gradient buffer itself (fp16 cast or fp32), not an encoded payload."""
        return _push_codecs()[self.codec].reducible

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self), sort_keys=True)


def add_arguments(ap: argparse.ArgumentParser) -> argparse.ArgumentParser:
    d = PSConfig()
    A = ap.add_argument
    A("--config", default="", help="JSON file with PSConfig fields")
    A("--mode", choices=["sync", "async"], default=None, help="Training mode (env SERVER_MODE)")
    A("--workers", type=int, default=None, help="Expected number of workers, 1-32 (env TOTAL_WORKERS_EXPECTED)")
    A("--lr", type=float, default=None, help="Learning rate (server SGD)")
    A("--port", type=int, default=None, help="Rendezvous port (env SERVER_PORT)")
    A("--staleness-bound", type=int, default=None, help="Maximum staleness accepted in async mode")
    A("--server", default=None, help="Server address host:port (env PARAMETER_SERVER_ADDRESS)")
    A("--worker-name", default=None, help="Worker name for identification")
    A("--epochs", type=int, default=None)
    A("--batch-size", type=int, default=None)
    A("--sync-steps", type=int, default=None, help="Local steps between push/fetch (reference semantics)")
    A("--accumulate", action="store_true", default=None,
      help="with --sync-steps K: push the mean gradient of all K batches of a window (reference: the first only)")
    A("--model", choices=["resnet18", "resnet50", "resnet_tiny"], default=None)
    A("--num-classes", type=int, default=None)
    A("--gpus", "--nproc", dest="gpus", type=int, default=None)
    A("--topology", choices=["colocated", "dedicated", "sharded"], default=None)
    A("--codec", choices=list(_push_codecs()), default=None,
      help="gradient wire: fp16 cast (reference, default), none (fp32), q8 (block-scaled int8, 1.016 B/param), "
           "sign1 (1-bit sign + a scale per 256, 0.1406 B/param) or topk; q8, sign1 and topk keep an error-feedback "
           "residual on the worker")
    A("--topk-ratio", type=float, default=None)
    A("--dtype", choices=["fp32", "bf16"], default=None,
      help="worker compute precision: fp32 (reference, default) or bf16 (fast path)")
    A("--momentum", type=float, default=None)
    A("--weight-decay", type=float, default=None)
    A("--optimizer", choices=["sgd", "lars", "adamw", "lamb"], default=None,
      help="server optimizer: sgd (default), lars (layer-wise trust ratio on tensors with ndim > 1; "
           "uses --momentum / --weight-decay; Python server, whole-arena updates), adamw (Adam with "
           "decoupled --weight-decay; Python server, also bucketed and sharded rounds) or lamb (the Adam "
           "moments with a per-tensor ratio |w| / |update| on tensors with ndim > 1; Python server, "
           "whole-arena updates)")
    A("--lars-trust", type=float, default=None, help="LARS trust coefficient (default 0.001)")
    A("--lars-eps", type=float, default=None, help="LARS denominator epsilon (default 1e-8)")
    A("--adam-beta1", type=float, default=None, help="AdamW / LAMB first-moment decay (default 0.9)")
    A("--adam-beta2", type=float, default=None, help="AdamW / LAMB second-moment decay (default 0.999)")
    A("--adam-eps", type=float, default=None, help="AdamW / LAMB denominator epsilon (default 1e-8)")
    A("--warmup-steps", type=int, default=None,
      help="linear warmup of the server learning rate: update k (1-based) runs with lr * min(1, k / N); "
           "0 = off (default); Python server only")
    A("--dc-lambda", type=float, default=None,
      help="async delay compensation (DC-ASGD): apply g + lambda*g*g*(w - w_at_fetch); 0 = off (default)")
    A("--dc-adaptive", action="store_true", default=None,
      help="with --dc-lambda: lambda / sqrt(running mean square of g + --dc-eps)")
    A("--dc-decay", type=float, default=None, help="--dc-adaptive: decay of the mean square (default 0.95)")
    A("--dc-eps", type=float, default=None, help="--dc-adaptive: epsilon under the square root (default 1e-7)")
    A("--clip-norm", type=float, default=None,
      help="clip the global L2 norm of the applied gradient to C (torch clip_grad_norm_ form; weight decay not "
           "clipped); 0 = off (default); implies --skip-nonfinite")
    A("--skip-nonfinite", action="store_true", default=None,
      help="skip a server update whose gradient sum holds inf / NaN (the round still counts)")
    A("--sync-semantics", choices=["barrier", "reference"], default=None)
    A("--bn-sync", action="store_true", default=None, help="workers push BN running stats; server averages")
    A("--deterministic", dest="deterministic", action="store_true", default=None,
      help="exact fixed-point BN statistic reductions: bit-reproducible training steps (the default; "
           "+0-2%% step time, profiles/r5_deterministic_ab.jsonl)")
    A("--no-deterministic", dest="deterministic", action="store_false", default=None,
      help="float-atomic BN statistic reductions (order-dependent rounding)")
    A("--fetch-codec", choices=["auto", "bf16conv", "fp32", "q8delta"], default=None,
      help="fetch wire: fp32 (the whole state), bf16conv (bf16 conv weights, --dtype bf16) or q8delta (sync, rank-0 "
           "server: one fp32 keyframe, then the block-scaled int8 of what changed since the workers' copy, 1.016 "
           "B/element with error feedback); auto = fp32 for --dtype fp32, bf16conv for --dtype bf16")
    A("--overlap", dest="overlap", action="store_true", default=None,
      help="sync mode: stream gradient buckets (reduce/apply/broadcast) during the backward pass")
    A("--no-overlap", dest="overlap", action="store_false", default=None)
    A("--bucket-mb", type=float, default=None, help="overlapped sync: gradient bucket size (MiB of fp16)")
    A("--synthetic", action="store_true", default=None)
    A("--synthetic-kind", choices=["proto", "hard"], default=None,
      help="synthetic data: proto (class prototype + noise) or hard (low contrast, 20%% label noise)")
    A("--data-dir", default=None, help="directory with cifar-100-binary/{train,test}.bin")
    A("--train-samples", type=int, default=None)
    A("--test-samples", type=int, default=None)
    A("--eval-every", type=int, default=None)
    A("--eval-workers", choices=["all", "first"], default=None,
      help="all: every worker evaluates the test set each epoch (reference); first: worker 0 only")
    A("--max-steps", type=int, default=None)
    A("--ckpt-every", type=int, default=None)
    A("--ckpt-dir", default=None)
    A("--resume", default=None)
    A("--seed", type=int, default=None)
    A("--heartbeat-timeout", type=float, default=None)
    A("--log-dir", default=None)
    A("--no-graph", dest="use_graph", action="store_false", default=None)
    A("--fault-inject", default=None,
      help="kill_worker:K@S, hang_worker:K@S[:secs] or crash_in_push:K@S (first attempt only)")
    A("--transfer-timeout", type=float, default=None,
      help="async server: seconds a gradient receive / snapshot send may stay in flight before the worker is "
           "dropped (its pair communicator aborted); 0 disables")
    A("--stall-timeout", type=float, default=None,
      help="async server: seconds a worker may send no request before it is dropped (catches a hung training "
           "loop whose heartbeat thread still runs); 0 disables")
    A("--round-timeout", type=float, default=None,
      help="sync rounds: seconds without a completed round before the communicator is aborted and the rank "
           "exits (status 3) for a launcher restart from the last checkpoint; 0 disables")
    A("--on-worker-loss", choices=["shrink", "restart"], default=None,
      help="sync, dedicated topology: shrink (default) = the surviving ranks rebuild the communicator and "
           "continue without the lost worker; restart = exit 3 for a launcher restart from the last checkpoint")
    A("--recovery-grace", type=float, default=None,
      help="shrink: seconds the server waits for the surviving ranks to check in (default: --round-timeout)")
    A("--verbose", type=int, default=None)
    return ap


def from_args(ns: argparse.Namespace) -> PSConfig:
    cfg = PSConfig()
    # environment defaults (reference env vars)
    cfg.mode = _env("SERVER_MODE", cfg.mode)
    cfg.workers = _env("TOTAL_WORKERS_EXPECTED", cfg.workers, int)
    cfg.port = _env("SERVER_PORT", cfg.port, int)
    cfg.server = _env("PARAMETER_SERVER_ADDRESS", cfg.server)
    # JSON config file
    if getattr(ns, "config", ""):
        with open(ns.config) as f:
            data = json.load(f)
        for k, v in data.items():
            if not hasattr(cfg, k):
                raise ValueError(f"unknown config key {k!r} in {ns.config}")
            setattr(cfg, k, v)
    # explicit CLI flags
    for f in dataclasses.fields(PSConfig):
        v = getattr(ns, f.name, None)
        if v is not None:
            setattr(cfg, f.name, v)
    return cfg.validate()


def parse(argv=None, description="psx parameter server") -> PSConfig:
    ap = add_arguments(argparse.ArgumentParser(description=description))
    return from_args(ap.parse_args(argv))
