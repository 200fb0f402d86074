"""The table of push codecs (parallel/pushcodec.py): what each entry answers, the recognition of a
pushed tensor, and the server's one round entry against the round methods named after how their
sources arrived."""
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.parallel import pushcodec as PC
from psx.parallel import q8 as Q
from psx.parallel import sign1 as S
from psx.parallel import topk as T
from psx.parallel.server import ParameterServer

from .test_ps_cpu import tiny_cfg

RATIO = 0.25


@pytest.mark.parametrize("name", ["none", "fp16", "topk", "q8", "sign1"])
def test_table_entry(name):
    n = 257
    c = PC.CODECS[name]
    dtype, size = {"none": (torch.float32, n), "fp16": (torch.float16, n),
                   "topk": (torch.int32, T.payload_words(T.topk_k(n, RATIO))),
                   "q8": (torch.uint8, Q.payload_bytes(n)), "sign1": (torch.uint8, S.payload_bytes(n))}[name]
    slot = c.slot(n, "cpu", RATIO)
    assert c.wire_dtype == dtype and slot.dtype == dtype and slot.numel() == size
    empty = c.empty(n, "cpu", RATIO)
    assert empty.dtype == dtype and empty.numel() == size
    out = torch.full((n,), 3.0)
    assert c.decode(empty, n, out, False, RATIO) is out and not out.any()
    assert PC.of_payload(empty, n) is c
    assert (c.encoder(n, "cpu", RATIO) is None) == (name in ("none", "fp16"))
    assert c.reducible == (name in ("none", "fp16"))
    assert PC.is_payload(empty) != c.reducible


def test_recognition():
    # an arena of 20 elements: one block, 16 + 16 + 32 bytes in both block wires
    assert Q.payload_bytes(20) == S.payload_bytes(20) == 64
    p = torch.zeros(64, dtype=torch.uint8)
    assert PC.of_payload(p, 20, "q8") is PC.CODECS["q8"]
    assert PC.of_payload(p, 20, "sign1") is PC.CODECS["sign1"]
    for prefer in (None, "fp16", "topk"):
        assert PC.of_payload(p, 20, prefer) is PC.CODECS["q8"]
    # n = 257, two blocks: the lengths (16 + 16 + 272 and 16 + 16 + 64 bytes) tell them apart,
    # whatever the configured codec
    assert (Q.payload_bytes(257), S.payload_bytes(257)) == (304, 96)
    for prefer in (None, "none", "fp16", "topk", "q8", "sign1"):
        assert PC.of_payload(torch.zeros(304, dtype=torch.uint8), 257, prefer) is PC.CODECS["q8"]
        assert PC.of_payload(torch.zeros(96, dtype=torch.uint8), 257, prefer) is PC.CODECS["sign1"]
        assert PC.of_payload(torch.zeros(9, dtype=torch.int32), 257, prefer) is PC.CODECS["topk"]
    with pytest.raises(ValueError, match="^a uint8 push of 300 bytes is neither a q8 nor a sign1 payload of 257 "
                                         "parameters$"):
        PC.of_payload(torch.zeros(300, dtype=torch.uint8), 257, "q8")


# ---------------------------------------------------------------------------- the round entry
N, W = 4097, 3


def _server():
    torch.manual_seed(4)
    m = torch.nn.Linear(N - 1, 1)
    lay = ParamLayout.from_module(m)
    assert lay.param_numel == N
    arena, counters = lay.pack(m)
    cfg = tiny_cfg(mode="sync", workers=W, codec="fp16", topk_ratio=RATIO, momentum=0.9)
    s = ParameterServer(cfg, lay, arena.clone(), counters, device="cpu", total_workers=W, log=lambda *a: None)
    for w in range(W):
        s.register_worker(f"w{w}", w)
    return s


def _sources(kind):
    """Two rounds' sources of each kind, from the same gradients."""
    gen = torch.Generator().manual_seed(8)
    enc = {"topk": [T.TopKCodec(N, RATIO) for _ in range(W)], "q8": [Q.Q8Codec(N) for _ in range(W)]}
    rounds = []
    for _ in range(2):
        g = [torch.randn(N, generator=gen) * 1e-2 for _ in range(W)]
        if kind == "reduced":
            rounds.append([(g[0].half() + g[1].half()) + g[2].half()])
        elif kind == "dense":
            rounds.append([x.half() for x in g])
        else:
            rounds.append([e.encode(x).clone() for e, x in zip(enc[kind], g)])
    return rounds


@pytest.mark.parametrize("legacy, kind", [("apply_reduced", "reduced"), ("apply_sources", "dense"),
                                          ("apply_gathered", "topk"), ("apply_payload_sources", "q8")])
def test_round_entry(legacy, kind):
    """Each round method named after how its sources arrived, and apply_round with the same
    sources, leave the same bits and the same counts; the second round runs the momentum form."""
    a, b = _server(), _server()
    members = list(range(W))
    for r, srcs in enumerate(_sources(kind)):
        steps = [r] * W
        if kind == "reduced":
            assert a.apply_reduced(srcs[0], members, steps)
            assert b.apply_round(srcs, members, steps, summed=True)
        else:
            assert getattr(a, legacy)(srcs, members, steps)
            assert b.apply_round(srcs, members, steps)
    assert a.core.global_step == b.core.global_step == 2
    per_worker = {"reduced": 2 * N, "dense": 2 * N, "topk": 4 * T.payload_words(T.topk_k(N, RATIO)),
                  "q8": Q.payload_bytes(N)}[kind]
    assert a.bytes_pushed == b.bytes_pushed == 2 * W * per_worker
    assert torch.equal(a.params.view(torch.int32), b.params.view(torch.int32))
    assert torch.equal(a.momentum_buf.view(torch.int32), b.momentum_buf.view(torch.int32))
    assert bool(a.momentum_buf.any()) and bool(torch.isfinite(a.params).all())
