"""Delta-quantised int8 fetch wire (fetch codec ``--fetch-codec q8delta``).

The push codecs (parallel/q8.py, parallel/sign1.py) shrink the worker-to-server half of a sync
round; this one shrinks the other half. Instead of the whole fp32 arena (4 bytes per element) a
fetch moves the block-scaled int8 of *what changed since the workers' copy*, 1.016 bytes per
element: two-way compression with error feedback, as in DoubleSqueeze (Tang et al. 2019).

* server: keeps ``shadow``, an fp32 array of arena_numel elements that holds exactly what every
  worker's ``local_arena`` holds. The first fetch of a job (and the first after an out-of-band
  change of the arena: resume) is a *keyframe*: the plain fp32 arena, ``shadow = arena``. Every
  later fetch encodes ``arena - shadow`` per block of 256 consecutive arena elements and advances
  ``shadow`` by what the payload decodes to — one streaming pass, csrc/kernels/q8.hip
  fetchq8_encode;
* wire: the payload of parallel/q8.py (``Q8B1``), unchanged, from the same quantiser
  (``q8.quantise``) in parallel/blockwire.py's frame;
* worker: ``local_arena = local_arena + deq``, which is ``q8.decode(add=True, scale=1.0)``.

The arithmetic is fixed so that the torch CPU path here and the HIP kernels agree bit for bit::

    d      = arena - shadow                  (one fp32 subtraction; the tail block is zero-filled)
    amax   = max |d|,  scale = amax / 127,  inv = 127 / amax if amax > 0 else 0
    q      = clamp(round_half_even(d * inv), -127, 127)      (a NaN product, 0 * inf, counts as 0)
    deq    = float(q) * scale                (one rounding)
    shadow = shadow + deq                    (a separate add, never an FMA)

A block holding a NaN or an Inf sends ``scale = NaN, q = 0``: ``shadow`` and every worker's copy of
that block go NaN alike, so a diverged run stays visible; the other blocks are unaffected.

Invariants: every worker's ``local_arena`` equals the server's ``shadow`` bit for bit at all times
(the worker-side add is the server-side add); the fp32 master stays on the server; what a round
fails to deliver is part of the next round's ``d``, so the error is fed back without a buffer of
its own and does not accumulate (a frozen arena is reached exactly after a few fetches).

A training step moves the BN running statistics inside the worker's ``local_arena``; the reference
fetch overwrites them, and so does this one: ``Receiver`` keeps the float-buffer region as
fetched and puts it back before the add.

Scope: sync rounds on a rank-0 server (``colocated`` / ``dedicated``) and the loopback. The async
loops would need a shadow per worker; bucketed rounds broadcast before the arena is final; the
native sync loop and the graph round speak the fp32 and bf16conv wires only (native_sync_enabled
and weight_image_enabled decline by their existing conditions); an aborted round may leave the
survivors in disagreement about whether the delta arrived, so elastic recovery takes the restart
path. There are no periodic keyframes.
"""
from __future__ import annotations

import torch

from . import blockwire as BW
from . import q8

payload_bytes = q8.payload_bytes
empty_payload = q8.empty_payload


def encode_into(arena: torch.Tensor, shadow: torch.Tensor, payload: torch.Tensor, n: int, off: int = 0, cnt=None):
    """Encode (arena - shadow)[off:off+cnt] into ``payload`` and leave shadow = shadow + deq there."""
    off, cnt = BW.check_range("q8", n, off, cnt)
    if shadow.device.type == "cuda":
        from ..ops import kernels as K

        K.fetchq8_encode(arena, shadow, payload, n, off, cnt)
        return payload
    q8.views(payload, n)
    if off == 0:
        BW.write_header(payload, q8.MAGIC, n)
    if cnt == 0:
        return payload
    sh = q8._blocks(shadow[off:off + cnt])
    scale, r, deq = q8.quantise(q8._blocks(arena[off:off + cnt] - shadow[off:off + cnt]))
    shadow[off:off + cnt] = (sh + deq).view(-1)[:cnt]
    q8.put(payload, n, off, cnt, scale, r)
    return payload


def apply(payload: torch.Tensor, local_arena: torch.Tensor, n: int, off: int = 0, cnt=None) -> torch.Tensor:
    """The worker side: local_arena[off:off+cnt] += deq(payload), the add ``encode_into`` did to shadow."""
    return q8.decode(payload, n, out=local_arena, scale=1.0, add=True, off=off, cnt=cnt)


class Receiver:
    """A worker's end of the wire: the receive buffer of the payload and the float-buffer region
    (BN running statistics) of the state as fetched, which the worker's steps overwrite in its
    ``local_arena``. ``version``: the server encode this copy stands at (in-process fetches)."""

    def __init__(self, layout, device="cpu"):
        self.n = layout.arena_numel
        self.np = layout.param_numel
        self.device = torch.device(device)
        self._payload = None
        self.bufs = None
        self.version = None

    @property
    def payload(self) -> torch.Tensor:
        """The receive buffer of a remote worker (an in-process one reads the server's payload)."""
        if self._payload is None:
            self._payload = empty_payload(self.n, self.device)
        return self._payload

    def keyframe(self, local_arena: torch.Tensor):
        """``local_arena`` has just received the whole fp32 state."""
        if self.bufs is None:
            self.bufs = torch.empty_like(local_arena[self.np:self.n])
        self.bufs.copy_(local_arena[self.np:self.n])

    def restore(self, local_arena: torch.Tensor):
        """``local_arena`` back to the state as last fetched (a step moved its BN statistics)."""
        if self.bufs is None:
            raise RuntimeError("q8delta: a delta fetch before the keyframe")
        if self.bufs.numel():
            local_arena[self.np:self.n].copy_(self.bufs)

    def apply(self, local_arena: torch.Tensor, payload: torch.Tensor | None = None):
        """local_arena (as last fetched) += deq of ``payload`` (default: the receive buffer)."""
        self.restore(local_arena)
        apply(self.payload if payload is None else payload, local_arena, self.n)
        self.bufs.copy_(local_arena[self.np:self.n])

    def state_sha256(self, local_arena: torch.Tensor) -> str:
        """sha256 of the state as fetched (equal to the server's ``fetch_shadow_sha256``)."""
        from .server import arena_sha256

        a = local_arena[: self.n].detach().clone()
        if self.bufs is not None and self.bufs.numel():
            a[self.np:].copy_(self.bufs)
        return arena_sha256(a)
