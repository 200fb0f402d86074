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

Blocks are independent, so every function takes a 256-aligned element sub-range ``off, cnt``.
"""
from __future__ import annotations

import torch

BLOCK = 256
MAGIC = 0x31423153  # the bytes 'S' '1' 'B' '1'
_FMAX = torch.finfo(torch.float32).max


def _pad16(x: int) -> int:
    return (x + 15) & ~15


def num_blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def section_offsets(n: int):
    """(byte offset of the scales, byte offset of the sign words, payload bytes)."""
    w_off = 16 + _pad16(4 * num_blocks(n))
    return 16, w_off, w_off + 32 * num_blocks(n)


def payload_bytes(n: int) -> int:
    return section_offsets(n)[2]


def views(payload: torch.Tensor, n: int):
    """(header int32[4], scales fp32[nblk], sign words int64[4 nblk]) views of a payload."""
    s_off, w_off, total = section_offsets(n)
    assert payload.dtype == torch.uint8 and payload.numel() == total, "not a sign1 payload of this n"
    return (payload[:16].view(torch.int32), payload[s_off:s_off + 4 * num_blocks(n)].view(torch.float32),
            payload[w_off:total].view(torch.int64))


def empty_payload(n: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros): a fresh encoder's buffer, and the
    dedicated server rank's slot in the gather."""
    p = torch.zeros(payload_bytes(n), dtype=torch.uint8, device=device)
    p[:16].view(torch.int32).copy_(torch.tensor([MAGIC, n, BLOCK, num_blocks(n)], dtype=torch.int32))
    return p


def _range(n: int, off: int, cnt):
    cnt = n - off if cnt is None else cnt
    if off % BLOCK or off < 0 or off + cnt > n or ((off + cnt) % BLOCK and off + cnt != n):
        raise ValueError("sign1 sub-range: 256-aligned start, end on a block boundary or at n")
    return off, cnt


def _blocks(flat: torch.Tensor) -> torch.Tensor:
    """[nb, 256] view of a flat fp32 range, the tail block zero-filled."""
    nb = num_blocks(flat.numel())
    if nb * BLOCK != flat.numel():
        flat = torch.cat([flat, flat.new_zeros(nb * BLOCK - flat.numel())])
    return flat.view(nb, BLOCK)


_LANES = torch.arange(64, dtype=torch.int64)


def encode_into(g: torch.Tensor, resid: torch.Tensor, payload: torch.Tensor, n: int, off: int = 0, cnt=None):
    """Encode (resid + g)[off:off+cnt] into ``payload`` and leave resid = acc - deq there."""
    off, cnt = _range(n, off, cnt)
    if resid.device.type == "cuda":
        from ..ops import kernels as K

        K.sign1_encode(g, resid, payload, n, off, cnt)
        return payload
    hdr, scales, words = views(payload, n)
    if off == 0:
        hdr.copy_(torch.tensor([MAGIC, n, BLOCK, num_blocks(n)], dtype=torch.int32))
    if cnt == 0:
        return payload
    acc = _blocks(resid[off:off + cnt] + g[off:off + cnt].to(torch.float32))
    nb = acc.shape[0]
    a = acc.abs()
    bad = (~(a <= _FMAX)).any(dim=1)  # NaN or Inf
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
    deq = torch.where(bit, -scale[:, None], scale[:, None])
    res = acc - deq
    resid[off:off + cnt] = res.view(-1)[:cnt]
    # word j of a block: bit l = sign of element 4 l + j (distinct bits: the sum is their or)
    wd = (bit.view(nb, 64, 4).to(torch.int64) << _LANES[None, :, None]).sum(dim=1)
    b0 = off // BLOCK
    words[4 * b0:4 * (b0 + nb)] = wd.view(-1)
    scales[b0:b0 + nb] = scale
    return payload


def decode(payload: torch.Tensor, n: int, out: torch.Tensor | None = None, scale: float = 1.0, add: bool = False,
           off: int = 0, cnt=None) -> torch.Tensor:
    """out[off:off+cnt] = [out +] scale * deq(payload); ``out`` defaults to a new zero tensor."""
    off, cnt = _range(n, off, cnt)
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
    v = deq * torch.tensor(scale, dtype=torch.float32)
    dst = out[off:off + cnt]
    if add:
        dst.add_(v)
    else:
        dst.copy_(v)
    return out


class Sign1Codec:
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
