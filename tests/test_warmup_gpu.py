"""--warmup-steps on the device: a W = 1 loopback server on resnet_tiny's layout (in-process
pushes, each applied straight from the wire through the collective rounds' kernel) with N = 4 ends
in the bits of the same run whose lr is set by hand before every round. The HIP engine does not
build resnet_tiny, so the gradients are synthetic wires."""
import pytest
import torch

from .test_warmup_cpu import grads, lr_of, tiny_server

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("opt", [dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4),
                                 dict(optimizer="adamw", weight_decay=1e-2),
                                 dict(optimizer="lars", momentum=0.9, weight_decay=5e-4),
                                 dict(optimizer="lamb", weight_decay=1e-2)],
                         ids=["sgd", "adamw", "lars", "lamb"])
def test_loopback_warmup_equals_lr_set_by_hand(opt):
    kw = dict(device=DEV, mode="sync", codec="fp16", dtype="bf16", **opt)
    a, lay = tiny_server(warmup_steps=4, **kw)
    b, _ = tiny_server(**kw)
    c, _ = tiny_server(**kw)  # constant lr: the warmup must change something
    for s in (a, b, c):
        s.enable_weight_wire()
    for k, g in enumerate(grads(lay.param_numel, 6), start=1):
        wire = g.half().to(DEV)
        b.lr = lr_of(k, 4)
        assert a.lr == b.lr
        for s in (a, b, c):
            assert s.push_gradients(0, wire, k)
    torch.cuda.synchronize()
    assert a.core.global_step == b.core.global_step == 6
    assert torch.equal(a.arena, b.arena) and not torch.equal(a.arena, c.arena)
    assert torch.equal(a.wire.img.view(torch.int16), b.wire.img.view(torch.int16))
    assert a.final_metrics()["final_param_sha256"] == b.final_metrics()["final_param_sha256"]
    if a.adam_m is not None:
        assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    if a.momentum_buf is not None:
        assert torch.equal(a.momentum_buf, b.momentum_buf)
