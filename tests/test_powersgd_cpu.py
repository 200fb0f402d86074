"""The PowerSGD codec (parallel/powersgd.py) on the CPU: its torch path against the method written
plainly in fp64 here, the payload's size, how a push is recognised, and the configuration's scope.
tests/test_powersgd_gpu.py runs the HIP kernels against the same reference."""
from types import SimpleNamespace as NS

import pytest
import torch

from psx.parallel import powersgd as PS
from psx.parallel import pushcodec as PC
from psx.parallel import q8, sign1, topk
from psx.utils.config import PSConfig

SHAPES = [(64, 27), (100, 512), (130, 1100), (8, 6), (37,)]
DROP = 1e-8
# The largest relative error of the same algorithm in fp32 torch on the CPU (the module's CPU path:
# another summation order) against the fp64 reference below, over both steps, ranks 4 and 8, fp32
# and fp16 gradients, on SHAPES: 2.28e-7 (products), 2.45e-7 (residuals), 1.96e-7 (orthogonality);
# the largest, times 8 for the MFMA's K order and the slab split.
TOL = 8 * 2.45e-7


def make_layout(shapes=SHAPES):
    entries, off = {}, 0
    for i, s in enumerate(shapes):
        numel = int(torch.Size(s).numel())
        entries[f"t{i}"] = NS(name=f"t{i}", region="param", offset=off, numel=numel, shape=tuple(s))
        off += numel
    return NS(entries=entries, param_numel=off)


def compressed(shape, rank):
    rows = shape[0]
    cols = int(torch.Size(shape).numel()) // rows
    return len(shape) > 1 and rank * (rows + cols) < rows * cols


def make_grads(layout, dtype, steps=2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(layout.param_numel, generator=gen).to(dtype) for _ in range(steps)]


class Reference:
    """The method of parallel/powersgd.py's docstring in fp64, one tensor after another."""

    def __init__(self, layout, rank, q0):
        self.layout, self.rank = layout, rank
        self.e = torch.zeros(layout.param_numel, dtype=torch.float64)
        self.q = {k: q.double().clone() for k, q in q0.items()}

    def step(self, g):
        """{name: (M, P^ Q'^T, P^)} of the compressed tensors; e and Q advance."""
        out = {}
        for k, t in self.layout.entries.items():
            if not compressed(t.shape, self.rank):
                continue
            rows = t.shape[0]
            sl = slice(t.offset, t.offset + t.numel)
            m = g[sl].double().view(rows, -1) + self.e[sl].view(rows, -1)
            p = m @ self.q[k]
            for j in range(self.rank):
                n0 = p[:, j] @ p[:, j]
                for i in range(j):
                    p[:, j] = p[:, j] - (p[:, i] @ p[:, j]) * p[:, i]
                n1 = p[:, j] @ p[:, j]
                p[:, j] = 0 if n1 == 0 or n1 <= DROP * n0 else p[:, j] / n1.sqrt()
            self.q[k] = m.t() @ p
            prod = p @ self.q[k].t()
            self.e[sl] = (m - prod).reshape(-1)
            out[k] = (m, prod, p)
        return out


def codec_q(codec):
    """{name: Q} of a codec's compressed tensors."""
    names = list(codec.layout.entries)
    return {names[k]: PS.factors_of(codec.table.seg[k], codec.q.cpu(), codec.rank)[1].clone() for k in codec.table.comp}


def check_step(codec, payload, ref_out, e_ref, tol=TOL):
    """One encode of ``codec`` against the reference's step: products, residuals, orthogonality."""
    names = list(codec.layout.entries)
    _, fac, _ = PS.views(payload.cpu(), codec.table)
    resid = codec.resid.cpu().double()
    for k in codec.table.comp:
        t = codec.layout.entries[names[k]]
        m, prod, _ = ref_out[names[k]]
        ph, qn = (x.double() for x in PS.factors_of(codec.table.seg[k], fac, codec.rank))
        sl = slice(t.offset, t.offset + t.numel)
        errs = ((ph @ qn.t() - prod).norm() / m.norm(), (resid[sl] - e_ref[sl]).norm() / m.norm(),
                (ph.t() @ ph - torch.eye(codec.rank, dtype=torch.float64)).abs().max())
        print(names[k], tuple(t.shape), [f"{float(x):.3g}" for x in errs])
        assert all(x <= tol for x in errs), (names[k], errs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("rank", [4, 8])
def test_cpu_path_matches_fp64(rank, dtype):
    layout = make_layout()
    codec = PS.PowerSGDCodec(layout, rank, seed=3, worker=1)
    ref = Reference(layout, rank, codec_q(codec))
    assert [compressed(s, rank) for s in SHAPES] == [True, True, True, False, False]
    dec = torch.zeros(layout.param_numel)
    for g in make_grads(layout, dtype):
        payload = codec.encode(g)
        check_step(codec, payload, ref.step(g), ref.e)
        PS.decode([payload], dec, layout, rank)
        for t in list(layout.entries.values())[3:]:  # the tail: fp16 of g, no residual
            sl = slice(t.offset, t.offset + t.numel)
            assert torch.equal(dec[sl], g[sl].half().float()) and not codec.resid[sl].any()


def test_payload_bytes_resnet18():
    from psx.models.layout import ParamLayout
    from psx.models.resnet import build_model

    layout = ParamLayout.from_module(build_model("resnet18", 10, seed=0))
    params = [e for e in layout.entries.values() if e.region == "param"]
    mats = [e for e in params if len(e.shape) > 1]
    # rows + cols over the 21 weight matrices of the 10-class model (with a 400-class head: 36,715)
    assert sum(e.shape[0] + e.numel // e.shape[0] for e in mats) == 36325
    tail = sum(e.numel for e in params if len(e.shape) == 1)
    want = 16 + 4 * 4 * 36325 + 2 * tail
    assert PS.payload_bytes(layout, 4) == (want + 15) // 16 * 16
    assert PS.empty_payload(layout, 4, "cpu").numel() == PS.payload_bytes(layout, 4)
    assert PS.payload_bytes(layout, 4) / layout.param_numel < 0.056


def test_of_payload():
    layout = make_layout()
    n, arg = layout.param_numel, PS.Binding(layout, 4, 0)
    pushes = {"powersgd": PS.empty_payload(layout, 4, "cpu"), "q8": q8.empty_payload(n, "cpu"),
              "sign1": sign1.empty_payload(n, "cpu"), "topk": topk.empty_payload(n, 0.01, "cpu"),
              "fp16": torch.zeros(n, dtype=torch.float16), "none": torch.zeros(n)}
    for name, t in pushes.items():
        assert PC.of_payload(t, n, "powersgd", arg) is PC.CODECS[name], name
    assert PC.is_payload(pushes["powersgd"]) and not PC.CODECS["powersgd"].reducible
    assert PC.CODECS["powersgd"].in_kernel is None


def test_config_scope():
    cfg = PSConfig(codec="powersgd").validate()
    assert cfg.powersgd_rank == 4 and not cfg.dense_wire and cfg.resolve_overlap(4) is False
    for bad in (dict(powersgd_rank=5), dict(topology="sharded"), dict(overlap=True)):
        with pytest.raises(ValueError):
            PSConfig(codec="powersgd", **bad).validate()
