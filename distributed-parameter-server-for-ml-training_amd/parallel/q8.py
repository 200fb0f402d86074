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
(what a bucketed round would encode and apply per bucket).
"""
from __future__ import annotations

import torch

BLOCK = 256
MAGIC = 0x31423851  # the bytes 'Q' '8' 'B' '1'
_FMAX = torch.finfo(torch.float32).max


def _pad16(x: int) -> int:
    return (x + 15) & ~15


def num_blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def section_offsets(n: int):
    """(byte offset of the scales, byte offset of q, payload bytes)."""
    q_off = 16 + _pad16(4 * num_blocks(n))
    return 16, q_off, q_off + _pad16(n)


def payload_bytes(n: int) -> int:
    return section_offsets(n)[2]


def views(payload: torch.Tensor, n: int):
    """(header int32[4], scales fp32[nblk], q int8[n]) views of a payload."""
    s_off, q_off, total = section_offsets(n)
    assert payload.dtype == torch.uint8 and payload.numel() == total, "not a q8 payload of this n"
    return (payload[:16].view(torch.int32), payload[s_off:s_off + 4 * num_blocks(n)].view(torch.float32),
            payload[q_off:q_off + n].view(torch.int8))


def empty_payload(n: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros): a fresh encoder's buffer, and the
    dedicated server rank's slot in the gather."""
    p = torch.zeros(payload_bytes(n), dtype=torch.uint8, device=device)
    p[:16].view(torch.int32).copy_(torch.tensor([MAGIC, n, BLOCK, num_blocks(n)], dtype=torch.int32))
    return p


def _range(n: int, off: int, cnt):
    cnt = n - off if cnt is None else cnt
    if off % BLOCK or off < 0 or off + cnt > n or ((off + cnt) % BLOCK and off + cnt != n):
        raise ValueError("q8 sub-range: 256-aligned start, end on a block boundary or at n")
    return off, cnt


def _blocks(flat: torch.Tensor) -> torch.Tensor:
    """[nb, 256] view of a flat fp32 range, the tail block zero-filled."""
    nb = num_blocks(flat.numel())
    if nb * BLOCK != flat.numel():
        flat = torch.cat([flat, flat.new_zeros(nb * BLOCK - flat.numel())])
    return flat.view(nb, BLOCK)


def encode_into(g: torch.Tensor, resid: torch.Tensor, payload: torch.Tensor, n: int, off: int = 0, cnt=None):
    """Encode (resid + g)[off:off+cnt] into ``payload`` and leave resid = acc - deq there."""
    off, cnt = _range(n, off, cnt)
    if resid.device.type == "cuda":
        from ..ops import kernels as K

        K.q8_encode(g, resid, payload, n, off, cnt)
        return payload
    hdr, scales, q = views(payload, n)
    if off == 0:
        hdr.copy_(torch.tensor([MAGIC, n, BLOCK, num_blocks(n)], dtype=torch.int32))
    if cnt == 0:
        return payload
    acc = _blocks(resid[off:off + cnt] + g[off:off + cnt].to(torch.float32))
    a = acc.abs()
    nonfinite = ~(a <= _FMAX)  # NaN or Inf
    bad = nonfinite.any(dim=1)
    amax = torch.where(nonfinite, torch.zeros_like(a), a).amax(dim=1)
    c127 = torch.full_like(amax, 127.0)
    scale = torch.where(bad, torch.full_like(amax, float("nan")), amax / c127)
    inv = torch.where(~bad & (amax > 0), c127 / amax, torch.zeros_like(amax))
    r = torch.round(acc * inv[:, None])
    r = torch.where(r.isnan(), torch.zeros_like(r), r).clamp_(-127.0, 127.0)
    deq = r * scale[:, None]
    res = acc - deq
    resid[off:off + cnt] = res.view(-1)[:cnt]
    q[off:off + cnt] = r.view(-1)[:cnt].to(torch.int8)
    b0 = off // BLOCK
    scales[b0:b0 + scale.numel()] = scale
    return payload


def decode(payload: torch.Tensor, n: int, out: torch.Tensor | None = None, scale: float = 1.0, add: bool = False,
           off: int = 0, cnt=None) -> torch.Tensor:
    """out[off:off+cnt] = [out +] scale * deq(payload); ``out`` defaults to a new zero tensor."""
    off, cnt = _range(n, off, cnt)
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=payload.device)
    if payload.device.type == "cuda":
        from ..ops import kernels as K

        K.q8_decode(payload, out, n, scale, add, off, cnt)
        return out
    _, scales, q = views(payload, n)
    b0, nb = off // BLOCK, num_blocks(cnt)
    deq = q[off:off + cnt].to(torch.float32) * scales[b0:b0 + nb].repeat_interleave(BLOCK)[:cnt]
    v = deq * torch.tensor(scale, dtype=torch.float32)
    dst = out[off:off + cnt]
    if add:
        dst.add_(v)
    else:
        dst.copy_(v)
    return out


class Q8Codec:
    """Worker-side encoder: owns the error-feedback residual and the payload buffer."""

    def __init__(self, n: int, device="cpu"):
        self.n = n
        self.device = torch.device(device)
        self.payload = empty_payload(n, self.device)
        self.resid = torch.zeros(n, dtype=torch.float32, device=self.device)

    @property
    def nbytes(self) -> int:
        return self.payload.numel()

    def encode(self, g: torch.Tensor) -> torch.Tensor:
        return encode_into(g[: self.n], self.resid, self.payload, self.n)
