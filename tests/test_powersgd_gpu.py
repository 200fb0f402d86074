"""The PowerSGD codec's HIP kernels (csrc/kernels/powersgd.hip) against the fp64 reference of
tests/test_powersgd_cpu.py on its layout: (64, 27); (100, 512), rows no multiple of 16; (130, 1100),
nothing a multiple of 64 and five slabs; (8, 6) and a 1-D tensor of 37 in the fp16 tail.

TOL is test_powersgd_cpu.py's: 8 x 2.45e-7, the largest relative error of the same algorithm in fp32
torch on the CPU against the fp64 reference on these shapes; the margin of 8 covers the MFMA's K
order and the slab split."""
import math

import pytest
import torch

from psx.parallel import powersgd as PS

from .test_powersgd_cpu import SHAPES, TOL, Reference, check_step, codec_q, compressed, make_grads, make_layout

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANKS = [4, 8]
DTYPES = [torch.float32, torch.float16]


def _bits(t):
    return t.cpu().view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", RANKS)
def test_two_encodes_match_fp64(rank, dtype):
    """Two consecutive encodes (the second with the warm Q and a non-zero e): products, residuals
    and orthogonality within TOL; error feedback closed, decode(payload) + e' == M within 2 ulp of
    the two terms, which holds only if the decode reproduces the worker's product bits; the tail is
    g.half() bit for bit and its e stays 0."""
    layout = make_layout()
    codec = PS.PowerSGDCodec(layout, rank, DEV, seed=3, worker=1)
    ref = Reference(layout, rank, codec_q(codec))
    names = list(layout.entries)
    dec = torch.full((layout.param_numel,), 7.0, device=DEV)
    for g in make_grads(layout, dtype):
        m32 = codec.resid.cpu() + g.float()  # fp32 M, as the kernel forms it
        payload = codec.encode(g.to(DEV))
        check_step(codec, payload, ref.step(g), ref.e)
        PS.decode([payload], dec, layout, rank)
        d, e = dec.cpu(), codec.resid.cpu()
        for name, shape in zip(names, SHAPES):
            t = layout.entries[name]
            sl = slice(t.offset, t.offset + t.numel)
            if compressed(shape, rank):
                bound = 2 * 2.0 ** -24 * (m32[sl].abs() + d[sl].abs())
                assert bool(((d[sl].double() + e[sl].double() - m32[sl].double()).abs() <= bound).all()), name
            else:
                assert torch.equal(d[sl], g[sl].half().float()) and not e[sl].any(), name
        _, _, tail = PS.views(payload.cpu(), codec.table)
        assert torch.equal(tail.view(torch.int16), g[-85:].half().view(torch.int16))


@pytest.mark.parametrize("case", ["zero", "rank1"])
def test_edge_inputs(case):
    layout = make_layout()
    codec = PS.PowerSGDCodec(layout, 4, DEV, seed=5)
    g = torch.zeros(layout.param_numel)
    if case == "rank1":
        gen = torch.Generator().manual_seed(1)
        for t in list(layout.entries.values())[:3]:
            rows = t.shape[0]
            g[t.offset:t.offset + t.numel] = torch.outer(torch.randn(rows, generator=gen),
                                                         torch.randn(t.numel // rows, generator=gen)).reshape(-1)
    payload = codec.encode(g.to(DEV))
    _, fac, _ = PS.views(payload.cpu(), codec.table)
    dec = PS.decode([payload], torch.empty(layout.param_numel, device=DEV), layout, 4).cpu()
    assert bool(torch.isfinite(fac).all() and torch.isfinite(dec).all() and torch.isfinite(codec.resid).all())
    assert bool(torch.isfinite(codec.q).all())
    if case == "zero":
        assert not fac.any() and not dec.any()
        return
    for t in list(layout.entries.values())[:3]:
        sl = slice(t.offset, t.offset + t.numel)
        assert (dec[sl].double() - g[sl].double()).norm() / g[sl].double().norm() <= TOL


@pytest.mark.parametrize("rank", RANKS)
def test_server_decode_three_workers(rank):
    """W = 3 against the fp64 sum of the payloads' own factors, overwrite and add, within the bound
    of a 3 r term fp32 dot product, (3 r + 2) 2^-24 sum |P^| |Q'|, plus for add the rounding of the
    last add; two runs give identical bits."""
    layout = make_layout()
    n = layout.param_numel
    payloads, want, mag = [], torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for w in range(3):
        codec = PS.PowerSGDCodec(layout, rank, DEV, seed=3, worker=w)
        g = make_grads(layout, torch.float32, steps=1, seed=10 + w)[0]
        payloads.append(codec.encode(g.to(DEV)).clone())
        _, fac, tail = PS.views(payloads[-1].cpu(), codec.table)
        for k, s in enumerate(codec.table.seg):
            sl = slice(int(s["offset"]), int(s["offset"] + s["numel"]))
            if s["comp"]:
                ph, qn = (x.double() for x in PS.factors_of(s, fac, rank))
                want[sl] += (ph @ qn.t()).reshape(-1)
                mag[sl] += (ph.abs() @ qn.abs().t()).reshape(-1)
            else:
                want[sl] += tail[int(s["foff"]):int(s["foff"] + s["numel"])].double()
                mag[sl] += tail[int(s["foff"]):int(s["foff"] + s["numel"])].double().abs()
    base = torch.randn(n, generator=torch.Generator().manual_seed(2))
    outs = []
    for _ in range(2):
        over = PS.decode(payloads, torch.full((n,), 9.0, device=DEV), layout, rank)
        added = PS.decode(payloads, base.to(DEV), layout, rank, add=True)
        outs.append((over, added))
        bound = (3 * rank + 2) * 2.0 ** -24 * mag
        assert bool(((over.cpu().double() - want).abs() <= bound).all())
        total = want + base.double()
        assert bool(((added.cpu().double() - total).abs() <= bound + 2.0 ** -24 * total.abs()).all())
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))


def test_loopback_run():
    from psx.models.layout import ParamLayout
    from psx.models.resnet import build_model
    from psx.parallel.runner import run_local
    from psx.utils.config import PSConfig

    cfg = PSConfig(model="resnet18", batch_size=64, epochs=1, train_samples=1024, eval_every=0, verbose=1, lr=0.05,
                   max_steps=3, mode="sync", workers=1, codec="powersgd").validate()
    out = run_local(cfg, log=lambda *a, **k: None)
    srv = out["server"]
    nbytes = PS.payload_bytes(ParamLayout.from_module(build_model("resnet18", cfg.num_classes, seed=0)), 4)
    assert srv["global_steps_completed"] == 3 and srv["bytes_pushed"] == 3 * nbytes
    assert math.isfinite(srv["final_param_checksum"]) and math.isfinite(out["workers"][0]["last_loss"])
