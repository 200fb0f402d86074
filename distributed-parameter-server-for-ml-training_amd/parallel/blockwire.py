"""The frame the block-scaled gradient wires share (parallel/q8.py, parallel/sign1.py and, through
q8, parallel/fetchq8.py; csrc/kernels/blockwire.hpp is the HIP side).

A payload is one fixed-size uint8 buffer for a given n::

    [ {magic, n, 256, nblk} int32 | fp32 scale[nblk], padded to 16 bytes | body ]

Blocks are runs of 256 consecutive arena elements (tensor boundaries are ignored) and are
independent, so every function takes a 256-aligned element sub-range ``off, cnt``. A codec module
keeps its arithmetic (how a ``[nb, 256]`` fp32 block array becomes scales and a body, and back) and
its body's size and dtype; everything else is here.
"""
from __future__ import annotations

import torch

BLOCK = 256
WIRE_DTYPE = torch.uint8
FMAX = torch.finfo(torch.float32).max


def pad16(x: int) -> int:
    return (x + 15) & ~15


def num_blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def section_offsets(n: int, body_bytes: int):
    """(byte offset of the scales, byte offset of the body, payload bytes)."""
    body_off = 16 + pad16(4 * num_blocks(n))
    return 16, body_off, body_off + body_bytes


def sections(payload: torch.Tensor, n: int, body_bytes: int, name: str):
    """(header int32[4], scales fp32[nblk], body uint8[body_bytes]) views of a payload."""
    s_off, body_off, total = section_offsets(n, body_bytes)
    assert payload.dtype == WIRE_DTYPE and payload.numel() == total, f"not a {name} payload of this n"
    return (payload[:16].view(torch.int32), payload[s_off:s_off + 4 * num_blocks(n)].view(torch.float32),
            payload[body_off:total])


def write_header(payload: torch.Tensor, magic: int, n: int):
    payload[:16].view(torch.int32).copy_(torch.tensor([magic, n, BLOCK, num_blocks(n)], dtype=torch.int32))


def empty_payload(magic: int, nbytes: int, n: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros): a fresh encoder's buffer, and the
    dedicated server rank's slot in the gather."""
    p = torch.zeros(nbytes, dtype=WIRE_DTYPE, device=device)
    write_header(p, magic, n)
    return p


def check_range(name: str, n: int, off: int, cnt):
    cnt = n - off if cnt is None else cnt
    if off % BLOCK or off < 0 or off + cnt > n or ((off + cnt) % BLOCK and off + cnt != n):
        raise ValueError(f"{name} sub-range: 256-aligned start, end on a block boundary or at n")
    return off, cnt


def blocks(flat: torch.Tensor) -> torch.Tensor:
    """[nb, 256] view of a flat fp32 range, the tail block zero-filled."""
    nb = num_blocks(flat.numel())
    if nb * BLOCK != flat.numel():
        flat = torch.cat([flat, flat.new_zeros(nb * BLOCK - flat.numel())])
    return flat.view(nb, BLOCK)


def nonfinite(a: torch.Tensor) -> torch.Tensor:
    """Mask of the NaN and Inf entries of ``a = |block|``."""
    return ~(a <= FMAX)


def store(out: torch.Tensor, off: int, cnt: int, deq: torch.Tensor, scale: float, add: bool):
    """out[off:off+cnt] = [out +] scale * deq, the product rounded before the add."""
    v = deq * torch.tensor(scale, dtype=torch.float32)
    dst = out[off:off + cnt]
    if add:
        dst.add_(v)
    else:
        dst.copy_(v)
    return out


class Encoder:
    """Worker-side encoder of a block wire (``wire``: parallel/q8.py or parallel/sign1.py): owns
    the error-feedback residual and the payload buffer."""

    def __init__(self, n: int, device="cpu"):
        self.n = n
        self.device = torch.device(device)
        self.payload = self.wire.empty_payload(n, self.device)
        self.resid = torch.zeros(n, dtype=torch.float32, device=self.device)

    @property
    def nbytes(self) -> int:
        return self.payload.numel()

    def encode(self, g: torch.Tensor) -> torch.Tensor:
        return self.wire.encode_into(g[: self.n], self.resid, self.payload, self.n)
