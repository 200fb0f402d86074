"""Block-scaled int8 gradient compression with error feedback (push codec ``--codec q8``).

The middle option between the reference's fp16 cast (2 bytes per parameter, parallel/codec.py)
and top-k sparsification (parallel/topk.py): every coordinate is still updated every round, at
1.016 bytes per parameter.

* worker: ``acc = resid + g``; per block of 256 consecutive arena elements (tensor boundaries
  are ignored) send ``scale = max|acc| / 127`` and ``q = round(acc / scale)`` as int8; keep
  ``resid = acc - q * scale`` (error feedback) — one streaming pass, csrc/kernels/q8.hip;
* wire: one fixed-size uint8 payload
  ``[ {magic 'Q8B1', n, 256, nblk} int32 | fp32 scale[nblk] | int8 q[n] ]``, the two sections
  padded to 16 bytes;
* server: the update kernel decodes and sums the W gathered payloads in fp32 in worker order
  inside the update itself (kernels.q8_apply_multi: no dense staging buffer, no scatter);
  ``decode`` serves the in-process accumulation and ``--sync-semantics reference``.

The arithmetic is fixed so that the torch CPU path here and the HIP kernels agree bit for bit::

    amax  = max |acc|                      (the tail block is zero-filled)
    scale = amax / 127,  inv = 127 / amax if amax > 0 else 0
    q     = clamp(round_half_even(acc * inv), -127, 127)     (a NaN product, 0 * inf, counts as 0)
    deq   = float(q) * scale               (one rounding)
    resid = acc - deq                      (a separate subtraction, never an FMA)

A block holding a NaN or an Inf sends ``scale = NaN, q = 0`` (its residual stays NaN): the
server's parameters go NaN as with the fp16 wire. Decode-and-sum over sources is
``s = 0; s = s + float(q_k) * scale_k`` in source order, the product rounded before the add.

Blocks are independent, so every function takes a 256-aligned element sub-range ``off, cnt``
(what a bucketed round would encode and apply per bucket). The payload's frame is
parallel/blockwire.py's; here are the quantiser, its inverse and the body's layout.
"""
from __future__ import annotations

import sys

import torch

from . import blockwire as BW
from .blockwire import BLOCK, num_blocks

MAGIC = 0x31423851  # the bytes 'Q' '8' 'B' '1'
_blocks = BW.blocks


def section_offsets(n: int):
    """(byte offset of the scales, byte offset of q, payload bytes)."""
    return BW.section_offsets(n, BW.pad16(n))


def payload_bytes(n: int) -> int:
    return section_offsets(n)[2]


def views(payload: torch.Tensor, n: int):
    """(header int32[4], scales fp32[nblk], q int8[n]) views of a payload."""
    hdr, scales, body = BW.sections(payload, n, BW.pad16(n), "q8")
    return hdr, scales, body[:n].view(torch.int8)


def empty_payload(n: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros)."""
    return BW.empty_payload(MAGIC, payload_bytes(n), n, device)


def quantise(blk: torch.Tensor):
    """[nb, 256] fp32 blocks -> (scale [nb], r [nb, 256] = float(q), deq [nb, 256]), by the
    arithmetic of the module docstring."""
    a = blk.abs()
    nonfinite = BW.nonfinite(a)
    bad = nonfinite.any(dim=1)
    amax = torch.where(nonfinite, torch.zeros_like(a), a).amax(dim=1)
    c127 = torch.full_like(amax, 127.0)
    scale = torch.where(bad, torch.full_like(amax, float("nan")), amax / c127)
    inv = torch.where(~bad & (amax > 0), c127 / amax, torch.zeros_like(amax))
    r = torch.round(blk * inv[:, None])
    r = torch.where(r.isnan(), torch.zeros_like(r), r).clamp_(-127.0, 127.0)
    return scale, r, r * scale[:, None]


def put(payload: torch.Tensor, n: int, off: int, cnt: int, scale: torch.Tensor, r: torch.Tensor):
    """The host encoders' write of a quantised range: its scales and int8 values."""
    _, scales, q = views(payload, n)
    q[off:off + cnt] = r.view(-1)[:cnt].to(torch.int8)
    b0 = off // BLOCK
    scales[b0:b0 + scale.numel()] = scale


def encode_into(g: torch.Tensor, resid: torch.Tensor, payload: torch.Tensor, n: int, off: int = 0, cnt=None):
    """Encode (resid + g)[off:off+cnt] into ``payload`` and leave resid = acc - deq there."""
    off, cnt = BW.check_range("q8", n, off, cnt)
    if resid.device.type == "cuda":
        from ..ops import kernels as K

        K.q8_encode(g, resid, payload, n, off, cnt)
        return payload
    views(payload, n)
    if off == 0:
        BW.write_header(payload, MAGIC, n)
    if cnt == 0:
        return payload
    acc = _blocks(resid[off:off + cnt] + g[off:off + cnt].to(torch.float32))
    scale, r, deq = quantise(acc)
    resid[off:off + cnt] = (acc - deq).view(-1)[:cnt]
    put(payload, n, off, cnt, scale, r)
    return payload


def decode(payload: torch.Tensor, n: int, out: torch.Tensor | None = None, scale: float = 1.0, add: bool = False,
           off: int = 0, cnt=None) -> torch.Tensor:
    """out[off:off+cnt] = [out +] scale * deq(payload); ``out`` defaults to a new zero tensor."""
    off, cnt = BW.check_range("q8", n, off, cnt)
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=payload.device)
    if payload.device.type == "cuda":
        from ..ops import kernels as K

        K.q8_decode(payload, out, n, scale, add, off, cnt)
        return out
    _, scales, q = views(payload, n)
    b0, nb = off // BLOCK, num_blocks(cnt)
    deq = q[off:off + cnt].to(torch.float32) * scales[b0:b0 + nb].repeat_interleave(BLOCK)[:cnt]
    return BW.store(out, off, cnt, deq, scale, add)


class Q8Codec(BW.Encoder):
    wire = sys.modules[__name__]
