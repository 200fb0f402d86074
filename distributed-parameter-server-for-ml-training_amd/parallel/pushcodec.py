"""The table of push codecs: one object per ``--codec`` value, which the worker, the channels, the
runner and the server ask instead of telling the codecs apart themselves.

    none   fp32 wire                         parallel/codec.py
    fp16   fp16 wire (the reference's cast)  parallel/codec.py
    topk   (index, fp16 value) pairs, int32  parallel/topk.py
    q8     block-scaled int8, uint8          parallel/q8.py
    sign1  block-scaled sign bits, uint8     parallel/sign1.py

An entry answers: ``wire_dtype``; ``slot``, the receive buffer of one push; ``empty``, the
contribution of a rank with no gradient; ``encoder``, the worker's error-feedback encoder or None;
``reducible``, whether a reduce can sum the wire (else it is gathered); ``wire_bytes``, the bytes one
push moves; ``decode``, the payload into dense fp32; ``in_kernel``, the name of the ops/kernels.py
wrapper that decodes such payloads inside the update (``Rule.device_payload``), or None. ``ratio``
is ``--topk-ratio``; only top-k reads it.

``of_payload`` recognises a pushed tensor on the host, never by reading a device header back: a
server takes whatever codec a push arrives in, whatever it is configured for.
"""
from __future__ import annotations

import torch

from . import blockwire, q8, sign1, topk


class Dense:
    reducible, in_kernel = True, None

    def __init__(self, name: str, wire_dtype):
        self.name, self.wire_dtype = name, wire_dtype

    def slot(self, n: int, device, ratio=None) -> torch.Tensor:
        return torch.empty(n, dtype=self.wire_dtype, device=device)

    def empty(self, n: int, device, ratio=None) -> torch.Tensor:
        return torch.zeros(n, dtype=self.wire_dtype, device=device)

    def encoder(self, n: int, device, ratio=None):
        return None

    def wire_bytes(self, t: torch.Tensor, n: int) -> int:
        return min(n, t.numel()) * t.element_size()

    def decode(self, payload, n: int, out: torch.Tensor, add: bool = False, ratio=None) -> torch.Tensor:
        return out.add_(payload[:n].to(torch.float32)) if add else out.copy_(payload[:n])


class TopK(Dense):
    reducible = False

    def slot(self, n, device, ratio=None):
        return torch.empty(topk.payload_words(topk.topk_k(n, ratio)), dtype=torch.int32, device=device)

    def empty(self, n, device, ratio=None):
        return topk.empty_payload(n, ratio, device)

    def encoder(self, n, device, ratio=None):
        return topk.TopKCodec(n, ratio, device)

    def wire_bytes(self, t, n):
        return t.numel() * 4

    def decode(self, payload, n, out, add=False, ratio=None):
        if not add:
            out.zero_()
        return topk.decode_add(payload, out, 1.0, topk.topk_k(n, ratio))


class Block(Dense):
    """A block wire of parallel/blockwire.py's frame (``wire``: its module)."""
    reducible, wire_dtype = False, blockwire.WIRE_DTYPE

    def __init__(self, name: str, wire, encoder, in_kernel: str):
        self.name, self.wire, self._encoder, self.in_kernel = name, wire, encoder, in_kernel

    def slot(self, n, device, ratio=None):
        return torch.empty(self.wire.payload_bytes(n), dtype=self.wire_dtype, device=device)

    def empty(self, n, device, ratio=None):
        return self.wire.empty_payload(n, device)

    def encoder(self, n, device, ratio=None):
        return self._encoder(n, device)

    def wire_bytes(self, t, n):
        return t.numel()

    def decode(self, payload, n, out, add=False, ratio=None):
        return self.wire.decode(payload, n, out=out, add=add)


CODECS = {"none": Dense("none", torch.float32), "fp16": Dense("fp16", torch.float16),
          "topk": TopK("topk", torch.int32),
          "q8": Block("q8", q8, q8.Q8Codec, "q8_apply_multi"),
          "sign1": Block("sign1", sign1, sign1.Sign1Codec, "sign1_apply_multi")}
_BLOCK = (CODECS["q8"], CODECS["sign1"])


def is_payload(t: torch.Tensor) -> bool:
    """A top-k or block-wire payload, which no reduce can sum, not a dense wire."""
    return t.dtype == torch.int32 or t.dtype == torch.uint8


def of_payload(t: torch.Tensor, n: int, prefer: str | None = None):
    """The codec of a pushed tensor for n parameters: int32 is top-k; uint8 is a block wire, told by
    its byte length, the ``prefer``-red (configured) codec's first where an arena of a few elements
    gives both the same; anything else is the dense wire of its dtype."""
    if t.dtype == torch.int32:
        return CODECS["topk"]
    if t.dtype == torch.uint8:
        own = CODECS.get(prefer)
        for c in ((own,) if own in _BLOCK else ()) + _BLOCK:
            if t.numel() == c.wire.payload_bytes(n):
                return c
        raise ValueError(f"a uint8 push of {t.numel()} bytes is neither a q8 nor a sign1 payload of "
                         f"{n} parameters")
    return CODECS["fp16"] if t.dtype == torch.float16 else CODECS["none"]
