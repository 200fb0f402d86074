"""1-bit sign gradient codec (parallel/sign1.py) on the CPU path: wire format, the fixed
arithmetic's properties, error feedback, server decode, and end-to-end PS runs (loopback + gloo)
with --codec sign1."""
import numpy as np
import pytest
import torch

from psx.models.layout import ParamLayout
from psx.models.resnet import TinyResNet
from psx.parallel import sign1 as S
from psx.parallel.runner import run_local
from psx.parallel.server import ParameterServer
from psx.utils.config import PSConfig

from .test_ps_cpu import TINY, _spawn, tiny_cfg
from .test_q8_cpu import make_grads

FMAX = torch.finfo(torch.float32).max


def tiny_n() -> int:
    return ParamLayout.from_module(TinyResNet(10)).param_numel


@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_format(n):
    nblk = -(-n // 256)
    pad = lambda x: -(-x // 16) * 16  # noqa: E731
    assert S.BLOCK == 256 and S.num_blocks(n) == nblk
    assert S.section_offsets(n) == (16, 16 + pad(4 * nblk), 16 + pad(4 * nblk) + 32 * nblk)
    assert S.payload_bytes(n) == 16 + pad(4 * nblk) + 32 * nblk and S.payload_bytes(n) % 16 == 0
    e = S.empty_payload(n, "cpu")
    assert e.dtype == torch.uint8 and e.numel() == S.payload_bytes(n)
    assert bytes(e[:4].tolist()) == b"S1B1"
    assert e[:16].view(torch.int32).tolist() == [S.MAGIC, n, 256, nblk]
    assert not e[16:].any() and not S.decode(e, n).any()
    c = S.Sign1Codec(n)
    assert c.nbytes == S.payload_bytes(n)
    p = c.encode(torch.randn(n))
    hdr, scales, words = S.views(p, n)
    assert hdr.tolist() == [S.MAGIC, n, 256, nblk] and scales.numel() == nblk
    assert words.dtype == torch.int64 and words.numel() == 4 * nblk
    assert scales.data_ptr() - p.data_ptr() == 16 and words.data_ptr() - p.data_ptr() == 16 + pad(4 * nblk)
    # the padding of the scales section stays zero; the sign words end the payload
    assert not p[16 + 4 * nblk:16 + pad(4 * nblk)].any()
    assert words.data_ptr() - p.data_ptr() + 8 * words.numel() == p.numel()


def test_payload_bytes_resnet18():
    assert S.payload_bytes(11_220_132) == 1_577_872


def wire_bits(words: torch.Tensor, n: int) -> torch.Tensor:
    """The sign bit of every element, read from the sign words by the stated order: element r of
    block b is bit r // 4 of word 4 b + r % 4."""
    w = words.numpy().view(np.uint64)
    i = np.arange(n)
    b, r = i // 256, i % 256
    return torch.from_numpy(((w[4 * b + r % 4] >> (r // 4).astype(np.uint64)) & np.uint64(1)).astype(bool))


def butterfly_sum(t: np.ndarray) -> np.ndarray:
    """Lane 0 of the xor butterfly over 64 lanes, offsets 32, 16, 8, 4, 2, 1, in fp32."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        t = (t + t[:, lanes ^ o]).astype(np.float32)
    return t[:, 0]


def check_step(acc: torch.Tensor, payload: torch.Tensor, resid: torch.Tensor, n: int, bad_expected=None):
    """The encode properties of one step, computed here from the step's fp32 input
    ``acc = resid_before + float(g)`` (CPU tensors) — not through the codec's own reference.
    Returns the mask of the non-finite blocks."""
    hdr, scales, words = S.views(payload, n)
    nblk = -(-n // 256)
    assert hdr.tolist() == [S.MAGIC, n, 256, nblk]
    a = torch.cat([acc, acc.new_zeros(nblk * 256 - n)]).view(nblk, 256)
    bad = (~(a.abs() <= FMAX)).any(1)
    if bad_expected is not None:
        assert bad.tolist() == bad_expected
    good = ~bad
    ok, bb = good.repeat_interleave(256)[:n], bad.repeat_interleave(256)[:n]
    # every bit equals acc < 0, in the stated word / bit order; the bits past n are 0
    bits = wire_bits(words, n)
    assert torch.equal(bits[ok], (acc < 0)[ok])
    tail_bits = wire_bits(words, nblk * 256)[n:]
    assert not tail_bits.any()
    # scale == the tree sum of the lanes' four-element sums divided by the count, exactly
    with np.errstate(all="ignore"):
        a4 = a.abs().numpy().reshape(nblk, 64, 4)
        t = (((a4[:, :, 0] + a4[:, :, 1]) + a4[:, :, 2]) + a4[:, :, 3]).astype(np.float32)
        cnt = np.full(nblk, 256.0, dtype=np.float32)
        if n % 256:
            cnt[-1] = n % 256
        want = torch.from_numpy((butterfly_sum(t) / cnt).astype(np.float32))
    assert torch.equal(scales[good], want[good])
    # resid is acc - deq with one rounding (evaluated in fp64)
    sc = scales.repeat_interleave(256)[:n]
    deq = torch.where(bits, -sc, sc)
    exact = acc.double() - deq.double()
    assert bool(((resid.double() - exact).abs()[ok] <= 2.0 ** -24 * exact.abs()[ok]).all())
    # per block: sum resid^2 <= sum acc^2 (the identity is sum acc^2 - cnt * scale^2; the margin
    # covers the fp32 roundings)
    pad0 = lambda x: torch.cat([x.double(), x.new_zeros(nblk * 256 - n).double()]).view(nblk, 256)  # noqa: E731
    r2, a2 = pad0(resid).square().sum(1), pad0(acc).square().sum(1)
    assert bool((r2[good] <= a2[good] * (1 + 1e-5)).all())
    # an all-zero block: scale 0, bits 0, decode 0
    zero = good & (a.abs().amax(1) == 0)
    zb = zero.repeat_interleave(256)[:n]
    dec = S.decode(payload.clone(), n)
    assert not scales[zero].any() and not bits[zb].any() and not dec[zb].any()
    assert torch.equal(dec[ok], deq[ok]) and bool(torch.isfinite(dec[ok]).all())
    # a block holding NaN or Inf: scale NaN, bits 0, NaN residual and decode for the whole block
    assert bool(scales[bad].isnan().all()) and not bits[bb].any()
    assert bool(resid[bb].isnan().all()) and bool(dec[bb].isnan().all())
    return bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n", [255, 257, 4097])
def test_encode_properties_chained(n, dtype):
    c = S.Sign1Codec(n)
    for g in make_grads(n, dtype):
        acc = c.resid + g.float()
        p = c.encode(g)
        assert not check_step(acc, p, c.resid, n).any()


def test_zero_and_nonfinite_blocks():
    """n = 4097 (17 blocks): block 1 all zero, a NaN in block 0 and an Inf in the last block at
    step 1. Those two send a NaN scale, zero bits and a NaN residual and stay poisoned at step 2;
    the other 15 pass every property (check_step masks nothing else)."""
    n = 4097
    c = S.Sign1Codec(n)
    for step, g in enumerate(make_grads(n, torch.float32, special=True)):
        acc = c.resid + g.float()
        p = c.encode(g)
        poisoned = step >= 1
        check_step(acc, p, c.resid, n, bad_expected=[poisoned] + [False] * 15 + [poisoned])
        _, scales, words = S.views(p, n)
        assert scales[1] == 0 and not words[4:8].any()
        assert bool(torch.isfinite(scales[1:-1]).all())


def test_subrange_encode_decode_matches_whole():
    n = 4097
    g = make_grads(n, torch.float32, steps=1)[0]
    whole, parts = S.Sign1Codec(n), S.Sign1Codec(n)
    whole.encode(g)
    S.encode_into(g, parts.resid, parts.payload, n, 0, 2048)
    S.encode_into(g, parts.resid, parts.payload, n, 2048, n - 2048)
    assert torch.equal(whole.payload, parts.payload) and torch.equal(whole.resid, parts.resid)
    out = torch.full((n,), 3.0)
    S.decode(whole.payload, n, out=out, scale=0.5, add=True, off=2048, cnt=n - 2048)
    ref = S.decode(whole.payload, n, out=torch.full((n,), 3.0), scale=0.5, add=True)
    assert torch.equal(out[2048:], ref[2048:]) and bool((out[:2048] == 3.0).all())
    with pytest.raises(ValueError):
        S.encode_into(g, parts.resid, parts.payload, n, 100, 256)
    with pytest.raises(ValueError):
        S.decode(whole.payload, n, off=256, cnt=100)


def _two_servers(codec_cfg, lay, arena, counters):
    out = []
    for _ in range(2):
        s = ParameterServer(codec_cfg, lay, arena.clone(), counters, total_workers=1, log=lambda *a: None)
        s.register_worker("w", 0)
        out.append(s)
    return out


def test_error_feedback_telescopes():
    """T pushes through Sign1Codec against the same gradients sent dense: sum_t deq_t =
    sum_t g_t - resid_T up to the codec's own roundings, so params_sign1 - lr * resid_T must equal
    params_dense up to
      * the fp32 rounding of the 2 * T updates and the final correction, each at most half an ulp
        of the parameter: (2 T + 2) / 2 ulps of the largest |p| (the term of
        test_q8_cpu.test_error_feedback_telescopes), and
      * unlike q8, whose resid + deq == acc exactly, two roundings per step in the codec,
        acc = fl(resid + g) and resid = fl(acc - deq), each at most 2^-24 A with A a bound of
        |acc| and |acc - deq|: |deq| = scale <= max |acc|, so |resid_t| <= 2 max |acc_t| and
        max |acc_t| <= 2 max |acc_(t-1)| + G with G = max |g|, hence A = 2 (2^T - 1) G; the 2 T
        roundings reach the parameters times lr: lr * 2 T * 2^-24 * A.
    Both terms are ~1e-6. A lost or double-counted residual is off by lr * |resid| ~ 1e-3 (checked
    below with a doubled residual)."""
    torch.manual_seed(3)
    T, lr = 8, 0.1
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    n = lay.param_numel
    cfg = tiny_cfg(mode="async", workers=1, codec="sign1", lr=lr)
    ss, sd = _two_servers(cfg, lay, arena, counters)
    enc = S.Sign1Codec(n)
    gen = torch.Generator().manual_seed(5)
    gmax = 0.0
    for _ in range(T):
        g = torch.randn(n, generator=gen) * 1e-2
        gmax = max(gmax, float(g.abs().max()))
        for s, wire in ((ss, None), (sd, g)):
            _, gs = s.fetch_parameters(0)
            assert s.push_gradients(0, enc.encode(g) if wire is None else wire, gs)
    assert ss.core.global_step == T and sd.core.global_step == T
    assert ss.bytes_pushed == T * S.payload_bytes(n)
    atol = ((2 * T + 2) / 2 * 2.0 ** -23 * float(sd.params.abs().max())
            + lr * 2 * T * 2.0 ** -24 * 2 * (2 ** T - 1) * gmax)
    assert atol < 1e-5
    assert torch.allclose(ss.params - lr * enc.resid, sd.params, rtol=0, atol=atol)
    assert not torch.allclose(ss.params - 2 * lr * enc.resid, sd.params, rtol=0, atol=atol)


@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_server_sign1_apply_matches_dense(mom):
    torch.manual_seed(1)
    m = TinyResNet(10)
    lay = ParamLayout.from_module(m)
    arena, counters = lay.pack(m)
    n = lay.param_numel
    cfg = tiny_cfg(mode="async", workers=1, codec="sign1", momentum=mom)
    s1, s2 = _two_servers(cfg, lay, arena, counters)
    enc = S.Sign1Codec(n)
    for _ in range(2):  # the second push exercises the momentum buffer
        p = enc.encode(torch.randn(n))
        dense = S.decode(p, n)
        for s, wire in ((s1, p), (s2, dense)):
            _, gs = s.fetch_parameters(0)
            assert s.push_gradients(0, wire, gs)
    assert torch.equal(s1.arena, s2.arena)
    assert not torch.equal(s1.arena, arena)


@pytest.mark.parametrize("mode,workers", [("sync", 2), ("async", 3)])
def test_run_local_sign1(mode, workers):
    cfg = tiny_cfg(mode=mode, workers=workers, codec="sign1", eval_every=0)
    res = run_local(cfg, log=lambda *a, **k: None)
    srv = res["server"]
    steps = -(-(96 // workers) // 8)
    assert srv["gradients_processed"] == workers * steps
    assert srv["bytes_pushed"] == srv["gradients_processed"] * S.payload_bytes(tiny_n())


def test_run_local_sign1_reference_semantics():
    cfg = tiny_cfg(mode="sync", workers=2, codec="sign1", eval_every=0, sync_semantics="reference")
    srv = run_local(cfg, log=lambda *a, **k: None)["server"]
    assert srv["global_steps_completed"] > 0
    assert srv["bytes_pushed"] == srv["gradients_processed"] * S.payload_bytes(tiny_n())


@pytest.mark.parametrize("args", [["--mode", "sync"], ["--mode", "sync", "--topology", "dedicated"],
                                  ["--mode", "async", "--staleness-bound", "50"]])
def test_dist_sign1_gloo(args):
    recs, _ = _spawn(3, args + ["--codec", "sign1"] + TINY)
    srv = [r for r in recs if r["type"] == "SERVER_FINAL_METRICS"][0]
    assert srv["global_steps_completed"] > 0 and srv["gradients_processed"] > 0
    assert srv["bytes_pushed"] == srv["gradients_processed"] * S.payload_bytes(tiny_n())


@pytest.mark.parametrize("kw", [dict(optimizer="adamw", lr=1e-3), dict(optimizer="lars", lr=0.05),
                                dict(clip_norm=1.0)])
def test_run_local_sign1_decoded_route(kw):
    """The rules without an in-kernel sign1 form take the decoded fp32 sum in the aggregation
    buffer: one run each, ending in finite parameters."""
    cfg = tiny_cfg(mode="sync", workers=2, codec="sign1", eval_every=0, **kw)
    res = run_local(cfg, log=lambda *a, **k: None)
    assert res["server"]["global_steps_completed"] > 0
    ck = res["server"]["final_param_checksum"]
    assert ck == ck and abs(ck) != float("inf")


def test_config_scope():
    with pytest.raises(ValueError):
        PSConfig(codec="sign1", topology="sharded").validate()
    with pytest.raises(ValueError):
        PSConfig(codec="sign2").validate()
    cfg = PSConfig(mode="sync", codec="sign1").validate()
    assert cfg.resolve_overlap(8) is False and not cfg.dense_wire
    assert PSConfig(mode="sync", codec="fp16").validate().resolve_overlap(8) is True
