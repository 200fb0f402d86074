"""Rank-r PowerSGD gradient compression with error feedback (push codec ``--codec powersgd``).

PowerSGD (Vogels et al. 2019) in a one-round-trip form that fits a parameter server: every worker
compresses on its own and the server sums the decoded products, so no second exchange is needed.
The worker keeps an fp32 residual ``e`` of the whole gradient and one ``cols x r`` matrix ``Q`` per
compressed tensor, drawn once from a generator seeded by ``--seed`` and the worker id and then
warm-started from every push. For every tensor with ndim > 1 and ``r (rows + cols) < rows cols``,
read as the row-major ``rows x cols`` matrix it is in the arena::

    M  = g + e
    P  = M Q
    P^ = the columns of P orthonormalised by modified Gram-Schmidt in column order
    Q' = M^T P^                         (the next push's Q)
    e  = M - P^ Q'^T
    wire: P^ and Q', fp32

A column of P whose squared norm after its projections is 0, or at most ``DROP`` of its squared
norm before them, travels as zeros, and so does its Q' column; the worker's Q keeps its previous
column then. Every other tensor travels as fp16 of ``g`` in a dense tail, without a residual,
exactly as the fp16 wire would send it.

* wire: one fixed-size uint8 payload ``[ {magic 'PSG1', n, rank, compressed tensors} int32 | fp32
  factors | fp16 tail ]`` padded to 16 bytes; a compressed tensor's factors are ``P^ [rows][r]``
  then ``Q' [cols][r]`` (ops/kernels.py PowerSGDTable holds the offsets). ResNet-18 at rank 4: 0.61
  MB instead of 22.4 MB of fp16;
* server: ``decode`` sums ``P^_w Q'_w^T`` over the W payloads in list order, and the fp16 tails in
  fp32, into the dense aggregation buffer; the configured update rule runs after that.

The HIP kernels are csrc/kernels/powersgd.hip; a CPU arena runs the same method in fp32 torch
(equal to a tolerance, not bit for bit: the summation orders differ).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from ..ops import kernels as K

MAGIC = 0x31475350  # the bytes 'P' 'S' 'G' '1'
DROP = 1e-8         # kPgDrop in csrc/kernels/powersgd.hip
HEADER = K.POWERSGD_HEADER


class Binding(NamedTuple):
    """What the codec's calls need beside n: the layout it is bound to, the rank, the seed of Q."""
    layout: object
    rank: int = 4
    seed: int = 0


_tables: dict = {}


def table(layout, rank: int, device="cpu") -> "K.PowerSGDTable":
    """The (cached) PowerSGDTable of a layout at a rank on a device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (id(layout), int(rank), str(device))
    hit = _tables.get(key)
    if hit is None or hit[0] is not layout:
        hit = _tables[key] = (layout, K.PowerSGDTable(layout, device, rank))
    return hit[1]


def payload_bytes(layout, rank: int) -> int:
    return table(layout, rank).payload_bytes


def empty_payload(layout, rank: int, device) -> torch.Tensor:
    """An all-zero payload with a header (decodes to zeros)."""
    tb = table(layout, rank)
    p = torch.zeros(tb.payload_bytes, dtype=torch.uint8)
    p[:HEADER].view(torch.int32).copy_(torch.tensor([MAGIC, tb.n, tb.rank, len(tb.comp)], dtype=torch.int32))
    return p.to(device)


def views(payload: torch.Tensor, tb):
    """(header int32[4], factors fp32, tail fp16) views of a payload of ``tb``."""
    assert payload.dtype == torch.uint8 and payload.numel() == tb.payload_bytes, "not a powersgd payload of this layout"
    f0 = HEADER + 4 * tb.factors
    return (payload[:HEADER].view(torch.int32), payload[HEADER:f0].view(torch.float32),
            payload[f0:f0 + 2 * tb.tails].view(torch.float16))


def orthonormalise(P: torch.Tensor) -> list:
    """Modified Gram-Schmidt of the columns of ``P`` in place, in column order; returns the dropped
    columns (stored as zeros)."""
    dropped = []
    for j in range(P.shape[1]):
        n0 = P[:, j].dot(P[:, j])
        for i in range(j):
            P[:, j] -= P[:, i].dot(P[:, j]) * P[:, i]
        n1 = P[:, j].dot(P[:, j])
        if n1 == 0 or n1 <= DROP * n0:
            P[:, j] = 0
            dropped.append(j)
        else:
            P[:, j] /= n1.sqrt()
    return dropped


def factors_of(seg, fac: torch.Tensor, rank: int):
    """(P^ [rows, r], Q' [cols, r]) views of one compressed tensor in a factor section."""
    rows, cols, f = int(seg["rows"]), int(seg["cols"]), int(seg["foff"])
    return fac[f:f + rows * rank].view(rows, rank), fac[f + rows * rank:f + (rows + cols) * rank].view(cols, rank)


def decode(payloads, out: torch.Tensor, layout, rank: int, add: bool = False) -> torch.Tensor:
    """out = [out +] the sum of the decoded payloads in list order (fp32)."""
    payloads = list(payloads)
    tb = table(layout, rank, out.device)
    if out.device.type == "cuda":
        K.powersgd_decode(payloads, out, tb, add)
        return out
    if not add:
        out[:tb.n].zero_()
    for p in payloads:
        _, fac, tail = views(p, tb)
        for s in tb.seg:
            o, n = int(s["offset"]), int(s["numel"])
            if s["comp"]:
                ph, qn = factors_of(s, fac, rank)
                out[o:o + n] += (ph @ qn.t()).reshape(-1)
            else:
                out[o:o + n] += tail[int(s["foff"]):int(s["foff"]) + n].float()
    return out


class PowerSGDCodec:
    """Worker-side encoder: owns the error-feedback residual, Q and the payload buffer."""

    def __init__(self, layout, rank: int = 4, device="cpu", seed: int = 0, worker: int = 0):
        self.layout, self.rank, self.seed = layout, int(rank), int(seed)
        self.device = torch.device(device)
        self.table = table(layout, rank, self.device)
        self.n = self.table.n
        self.payload = empty_payload(layout, rank, self.device)
        self.resid = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.ws = self.table.workspace() if self.device.type == "cuda" else None
        self.pushes = 0
        self.bind_worker(worker)

    def bind_worker(self, worker: int):
        """Draw Q for this worker id (before the first push: Q is never reset after it)."""
        assert self.pushes == 0, "powersgd: Q is drawn once, before the first push"
        tb = self.table
        gen = torch.Generator().manual_seed(1_000_003 * self.seed + int(worker))
        q = torch.zeros(max(1, tb.factors), dtype=torch.float32)
        for k in tb.comp:
            _, qk = factors_of(tb.seg[k], q, self.rank)
            qk.copy_(torch.randn(qk.shape, generator=gen))
        self.q = q.to(self.device)

    @property
    def nbytes(self) -> int:
        return self.payload.numel()

    def encode(self, g: torch.Tensor) -> torch.Tensor:
        g = g[: self.n]
        self.pushes += 1
        tb = self.table
        if self.device.type == "cuda":
            K.powersgd_encode(g.contiguous(), self.resid, self.q, self.payload, self.ws, tb)
            return self.payload
        _, fac, tail = views(self.payload, tb)
        for s in tb.seg:
            o, n = int(s["offset"]), int(s["numel"])
            if not s["comp"]:
                tail[int(s["foff"]):int(s["foff"]) + n] = g[o:o + n].to(torch.float16)
                continue
            e = self.resid[o:o + n].view(int(s["rows"]), int(s["cols"]))
            m = e.add_(g[o:o + n].to(torch.float32).view_as(e))
            ph, qn = factors_of(s, fac, self.rank)
            _, q = factors_of(s, self.q, self.rank)
            ph.copy_(m @ q)
            dropped = orthonormalise(ph)
            qn.copy_(m.t() @ ph)
            keep = [j for j in range(self.rank) if j not in dropped]
            q[:, keep] = qn[:, keep]
            e.sub_(ph @ qn.t())
        return self.payload
