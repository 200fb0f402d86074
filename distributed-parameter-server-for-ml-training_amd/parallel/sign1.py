"""1-bit sign gradient compression with error feedback (push codec ``--codec sign1``).

1-bit SGD with error feedback (Seide et al. 2014) in the scaled-sign form of EF-signSGD
(Karimireddy et al. 2019): every coordinate still moves every round, as with the fp16 cast
(parallel/codec.py) and block-scaled int8 (parallel/q8.py), at 0.1406 bytes per parameter.

* worker: ``acc = resid + g``; per block of 256 consecutive arena elements (tensor boundaries
  are ignored) send ``scale = mean|acc|`` and one sign bit per element; keep
  ``resid = acc -+ scale`` (error feedback) — one streaming pass, csrc/kernels/sign1.hip;
* wire: one fixed-size uint8 payload
  ``[ {magic 'S1B1', n, 256, nblk} int32 | fp32 scale[nblk] | uint64 signs[4 nblk] ]``, the scales
  section padded to 16 bytes. Word ``j`` (0..3) of a block has bit ``l`` (0..63) equal to the sign
  of block element ``4 l + j``: the lane that owns elements ``4 l .. 4 l + 3`` contributes bit
  ``l`` to each of four wave ballots;
* server: the update kernel decodes and sums the W gathered payloads in fp32 in worker order
  inside the update itself (kernels.sign1_apply_multi: no dense staging buffer, no scatter);
  ``decode`` serves every other rule, the in-process accumulation and
  ``--sync-semantics reference``.

The arithmetic is fixed so that the torch CPU path here and the HIP kernels agree bit for bit
(every multiply, add and subtract separate)::

    t_l   = ((|a[4l]| + |a[4l+1]|) + |a[4l+2]|) + |a[4l+3]|    (elements at or past n count as 0)
    sum   = xor-butterfly of t over the 64 lanes, offsets 32, 16, 8, 4, 2, 1
            (here: repeatedly t[:, :w] + t[:, w:2w] for w = 32..1 — same bits, the adds commute)
    scale = sum / float(cnt)               (cnt = 256, or n % 256 in a tail block)
    bit   = acc < 0                        (-0.0, +0.0 and NaN give 0)
    deq   = -scale if bit else scale
    resid = acc - deq

A block holding a NaN or an Inf sends ``scale = NaN`` and all bits 0 (its residual becomes NaN
for the whole block): the server's parameters go NaN as with the fp16 wire. Decode-and-sum over
sources is ``s = 0; s = s + deq_k`` in source order.

Blocks are independent, so every function takes a 256-aligned element sub-range ``off, cnt``. The
payload's frame is parallel/blockwire.py's; here are the sign coder, its inverse and the body's layout.
"""
from __future__ import annotations

import sys

import torch

from . import blockwire as BW
from .blockwire import BLOCK, num_blocks

MAGIC = 0x31423153  # the bytes 'S' '1' 'B' '1'


def section_offsets(n: int):
    """(byte offset of the scales, byte offset of the sign words, payload bytes)."""
    return BW.section_offsets(n, 32 * num_blocks(n))


def payload_bytes(n: int) -> int:
    return section_offsets(n)[2]


def views(payload: torch.Tensor, n: int):
    """(header int32[4], scales fp32[nblk], sign words int64[4 nblk]) views of a payload."""
    hdr, scales, body = BW.sections(payload, n, 32 * num_blocks(n), "sign1")
    return hdr, scales, body.view(torch.int64)


def empty_payload(n: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros)."""
    return BW.empty_payload(MAGIC, payload_bytes(n), n, device)


_LANES = torch.arange(64, dtype=torch.int64)


def quantise(acc: torch.Tensor, cnt: int):
    """[nb, 256] fp32 blocks holding cnt elements -> (scale [nb], bit [nb, 256], deq [nb, 256]),
    by the arithmetic of the module docstring."""
    nb = acc.shape[0]
    a = acc.abs()
    bad = BW.nonfinite(a).any(dim=1)
    a4 = a.view(nb, 64, 4)
    t = ((a4[:, :, 0] + a4[:, :, 1]) + a4[:, :, 2]) + a4[:, :, 3]
    w = 32
    while w >= 1:
        t = t[:, :w] + t[:, w:2 * w]
        w //= 2
    count = torch.full((nb,), float(BLOCK), dtype=torch.float32)
    if cnt % BLOCK:
        count[-1] = float(cnt % BLOCK)
    scale = torch.where(bad, torch.full_like(count, float("nan")), t[:, 0] / count)
    bit = (acc < 0) & ~bad[:, None]
    return scale, bit, torch.where(bit, -scale[:, None], scale[:, None])


def encode_into(g: torch.Tensor, resid: torch.Tensor, payload: torch.Tensor, n: int, off: int = 0, cnt=None):
    """Encode (resid + g)[off:off+cnt] into ``payload`` and leave resid = acc - deq there."""
    off, cnt = BW.check_range("sign1", n, off, cnt)
    if resid.device.type == "cuda":
        from ..ops import kernels as K

        K.sign1_encode(g, resid, payload, n, off, cnt)
        return payload
    _, scales, words = views(payload, n)
    if off == 0:
        BW.write_header(payload, MAGIC, n)
    if cnt == 0:
        return payload
    acc = BW.blocks(resid[off:off + cnt] + g[off:off + cnt].to(torch.float32))
    nb = acc.shape[0]
    scale, bit, deq = quantise(acc, cnt)
    resid[off:off + cnt] = (acc - deq).view(-1)[:cnt]
    # word j of a block: bit l = sign of element 4 l + j (distinct bits: the sum is their or)
    wd = (bit.view(nb, 64, 4).to(torch.int64) << _LANES[None, :, None]).sum(dim=1)
    b0 = off // BLOCK
    words[4 * b0:4 * (b0 + nb)] = wd.view(-1)
    scales[b0:b0 + nb] = scale
    return payload


def decode(payload: torch.Tensor, n: int, out: torch.Tensor | None = None, scale: float = 1.0, add: bool = False,
           off: int = 0, cnt=None) -> torch.Tensor:
    """out[off:off+cnt] = [out +] scale * deq(payload); ``out`` defaults to a new zero tensor."""
    off, cnt = BW.check_range("sign1", n, off, cnt)
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=payload.device)
    if payload.device.type == "cuda":
        from ..ops import kernels as K

        K.sign1_decode(payload, out, n, scale, add, off, cnt)
        return out
    if cnt == 0:
        return out
    _, scales, words = views(payload, n)
    b0, nb = off // BLOCK, num_blocks(cnt)
    bit = ((words[4 * b0:4 * (b0 + nb)].view(nb, 1, 4) >> _LANES[None, :, None]) & 1).bool()
    sc = scales[b0:b0 + nb].view(nb, 1, 1)
    deq = torch.where(bit, -sc, sc).reshape(-1)[:cnt]
    return BW.store(out, off, cnt, deq, scale, add)


class Sign1Codec(BW.Encoder):
    wire = sys.modules[__name__]
