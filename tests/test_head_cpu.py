"""The fp64 references of the classifier head (csrc/kernels/head.hip: psx_head_fwd_bwd on its fused
and split paths, the BN-backward sums of the fused kernel, psx_head_wgrad), the case tables, the
error bounds the kernels are held to, and the CPU tests that give the bounds their meaning: the
reference equals torch float64 autograd, the same formulas in torch fp32 stay inside every bound on
every case of the tables, and each wrong variant of WRONG leaves them. Everything public here is
shared with tests/test_head_gpu.py.

Conventions. act is [B, HW, C] (NHWC, pixels flattened), a ReLU output (>= 0); bf16 decodes
exactly. Every reference is float64, every bound is one float64 per output element, absolute in
the magnitudes of the terms (an element that cancels is held like its neighbours).

Bounds: standard forward error analysis with g(n) = n u / (1 - n u), u = 2^-24: an fp32 sum or dot
product of n terms in any order (sequential, 4-lane partials and shuffles, 32-wide GEMM chunks,
split-K float atomics) is within g(n) sum |terms|; a fused multiply-add only removes roundings.

  pooled    sum of HW terms, the rounded 1 / HW, one product      g(HW + 2) pooled
  logits z  b(pooled) carried through |w|, a C-term dot, the bias add (and up to 16 atomics, which
            are adds of the same terms)                            |w| b(pooled) + g(C + 4) (|p| |w| + |bias|)
  exp, log  __expf and __logf have no derivable constant. Each is modelled with a relative error of
            E u (|argument| + 1). The ROCm documentation installed with the toolchain states no
            accuracy for the native exp2 / log2 these expand to, so E = 2, the issue's start value.
  lse       mx + log S, S = sum_k exp(z_k - mx). lse is 1-Lipschitz in z (sup norm): max_k b(z_k).
            t_k = z_k - mx rounds once (u |t_k|, relative in exp), exp adds E u (|t_k| + 1), the
            K-term sum of positives g(K) relative; a flushed subnormal exp adds K 2^-126 / S.
            All of it is a relative error of S, so an absolute one of log S. log: E u (S + 1)
            |log S|; the add mx + log: u |lse|.
  loss      lse - z_y: b(lse) + b(z_y) + u |loss|
  dlogits   (exp(z_k - lse) - [k = y]) / B: p_k (b(z_k) + b(lse) + u |a_k| + E u (|a_k| + 1)) with
            a_k = z_k - lse, the subtraction, the rounded 1 / B and the product: 3 u |p_k - [k = y]|
  dact      sum_k dlogits_k w_kc / HW: |w| b(dlogits) + g(K + 3) |dlogits| |w|, all over HW; a bf16
            sink adds half an ulp of bf16 at the reference value (taken at |ref| + the bound so far:
            the value that is rounded may lie in the next binade)
  BN sums   per slot row, per-sample fp32 partials of HW terms of three roundings each, ceil(B / 8)
            atomics: g(HW + ceil(B / 8) + 4) sum |terms|. Deterministic mode replaces the atomics
            by exact integer adds: the same bound holds.
  dw, db    B-term dot / sum, gscale: g(B + 2), g(B + 1) on gscale sum |terms|; the fp16 sink adds
            half an ulp of fp16."""
import math

import pytest
import torch
import torch.nn.functional as F

from .test_bn_cpu import BF16, F32, SLOTS
from .test_lars_cpu import f32
from .test_sgd_cpu import U, assert_within, within

F16 = torch.float16
E = 2.0           # see the module docstring; profiles/head_paths.txt holds the measured ratios
TINY = 2.0 ** -126

# (B, HW, C, K): the smallest shapes that reach each branch (test_tables_reach_their_branches)
FUSED = ((1, 1, 16, 1), (3, 4, 64, 10), (9, 16, 512, 100), (19, 4, 256, 257), (2, 1, 256, 1024), (5, 4, 1024, 100))
SPLIT = ((33, 4, 320, 841), (1, 1, 1024, 264), (2, 4, 64, 4104), (3, 49, 768, 400))
TABLE = FUSED + SPLIT
REFUSED = ((16, 1025), (24, 10), (768, 10))  # (C, K)
NULL_CASE = (2, 1, 512, 1000)                # split-sized, runs fused when pooled is null
KINDS = ("plain", "wide", "tie", "edge_labels")
SUMS_CASES = tuple((B, 4, 64, 10) for B in (1, 8, 9, 19)) + ((9, 4, 1024, 100),)
WGRAD_SMALL = ((1, 1, 16), (33, 10, 48), (257, 100, 512))  # (B, K, C)
WGRAD_LARGE = ((33, 841, 320), (2, 4104, 64))
GSCALES = (1.0, 1.0 / 3.0)


# ---------------------------------------------------------------------------- host mirrors
def head_split(C, K, bufs=True):
    return K * C > (1 << 18) and C % 64 == 0 and bufs


def head_fused_ok(C, K):
    return not (K > 1024 or C % 16 or (C > 512 and C % 512))


def split_ks(C, det):
    return 1 if det else (16 if C >= 1024 else 4)


def split_ranges(Kd, ks):
    """[kbeg, kend) of every blockIdx.z of head_gemm_kernel (EPI 0)."""
    kper = -(-Kd // (ks * 32)) * 32
    return [(z * kper, min(Kd, z * kper + kper)) for z in range(ks)]


def wgrad_small(K, C):
    return K * C <= (1 << 18)


def g(n):
    return n * U / (1.0 - n * U)


def half_ulp(v, dtype):
    """Half the spacing of ``dtype`` at |v| (float64 tensor); 0 for fp32, which is the arithmetic."""
    if dtype == F32:
        return torch.zeros_like(v)
    p, emin = (8, -126) if dtype == BF16 else (11, -14)
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** emin))  # |v| = m 2^ex, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), (ex - 1).clamp_min(emin) - p)


# ---------------------------------------------------------------------------- inputs
def tied_rows(K):
    return sorted({K // 5, K // 2, K - 1}) if K >= 4 else list(range(K))


def head_inputs(B, HW, C, K, dtype, kind):
    """Seeded inputs, cached and shared (leave them unchanged): act (``dtype``, a ReLU output), w
    [K, C], bias [K], labels int32 [B]. Kinds: plain (logits of order 2); wide (the same, scaled so
    that the logits span +-40); tie (rows tied_rows(K) of w are zero and share one bias, 1 above
    every other logit of the batch: their logits are that bias exactly on every path; the label is
    the lowest tied, a middle tied, or a row that is not tied, by b % 3); edge_labels (labels 0 and
    K - 1). K < 4 has no three rows to tie: all its rows are."""
    key = (B, HW, C, K, dtype, kind)
    if key in head_inputs.cache:
        return head_inputs.cache[key]
    for attempt in range(16):  # reseeded until no sample's two largest logits are close
        seed = 977 + B + 3 * HW + 5 * C + 7 * K + 11 * KINDS.index(kind) + 1009 * attempt
        gen = torch.Generator().manual_seed(seed)
        act = torch.relu(torch.randn(B, HW, C, generator=gen)).to(dtype)
        w = torch.randn(K, C, generator=gen) * (3.0 / math.sqrt(C))
        bias = torch.randn(K, generator=gen) * 0.5
        labels = torch.randint(0, K, (B,), generator=gen, dtype=torch.int32)
        pooled = act.double().mean(1)
        if kind == "wide":
            z = pooled @ w.double().t() + bias.double()
            s = 40.0 / float(z.abs().max())
            w, bias = (w.double() * s).float(), (bias.double() * s).float()
        elif kind == "tie":
            T = tied_rows(K)
            w[T] = 0.0
            rest = [k for k in range(K) if k not in T]
            if rest:
                z = pooled @ w.double().t() + bias.double()
                bias[T] = f32(float(z[:, rest].max()) + 1.0)
            for b in range(B):
                labels[b] = (T[0], T[len(T) // 2], rest[0] if rest else T[0])[b % 3]
        elif kind == "edge_labels":
            labels = torch.tensor([0 if b % 2 == 0 else K - 1 for b in range(B)], dtype=torch.int32)
        z = pooled @ w.double().t() + bias.double()
        top = z.topk(min(2, K), 1).values
        if K == 1 or kind == "tie" or float((top[:, 0] - top[:, 1]).min()) > 1e-4 * (1 + float(z.abs().max())):
            break
    out = dict(B=B, HW=HW, C=C, K=K, dtype=dtype, kind=kind, act=act, w=w, bias=bias, labels=labels)
    head_inputs.cache[key] = out
    return out


head_inputs.cache = {}


def sums_inputs(B, HW, C, dtype):
    """y1 (the BN input of the layer the head consumes, ``dtype``) and saved [2, C] (mean, invstd)."""
    gen = torch.Generator().manual_seed(31 + B + 7 * C)
    y1 = torch.randn(B, HW, C, generator=gen).to(dtype)
    saved = torch.stack([0.1 * torch.randn(C, generator=gen), 1.0 + torch.rand(C, generator=gen)])
    return y1, saved


def wgrad_inputs(B, K, C, overflow=False):
    """dlogits [B, K] of order 1e-2 with mixed signs, pooled [B, C] in [0.05, 0.55]. ``overflow``:
    column 0 of dlogits is positive and scaled by 1e9, so dw[0, :] and db[0] are far past the
    largest fp16."""
    gen = torch.Generator().manual_seed(53 + B + 3 * K + 5 * C)
    dl = torch.randn(B, K, generator=gen) * 1e-2
    pooled = torch.rand(B, C, generator=gen) * 0.5 + 0.05
    if overflow:
        dl[:, 0] = dl[:, 0].abs() * 1e9 + 1e6
    return dl, pooled


# ---------------------------------------------------------------------------- references
def head_reference(inp):
    """(ref, bound): dicts of float64 under pooled [B, C], logits [B, K], loss [B], dlogits [B, K],
    dact [B, HW, C]; ref also holds arg [B] (lowest index among equal maxima), correct (int) and
    decided [B]: the maximum stands clear of every other logit by more than their bounds, so the
    count is exact for any evaluation inside the bounds."""
    B, HW, C, K, dtype = (inp[k] for k in ("B", "HW", "C", "K", "dtype"))
    a, w, bias = inp["act"].double(), inp["w"].double(), inp["bias"].double()
    y = inp["labels"].long()
    pooled = a.sum(1) / HW
    b_pooled = g(HW + 2) * pooled.abs()
    z = pooled @ w.t() + bias
    b_z = b_pooled @ w.abs().t() + g(C + 4) * (pooled.abs() @ w.abs().t() + bias.abs())
    mx = z.max(1, keepdim=True).values
    idx = torch.arange(K).expand(B, K)
    arg = torch.where(z == mx, idx, torch.full_like(idx, K)).min(1).values
    below = torch.where(z < mx, z, torch.full_like(z, -math.inf)).max(1).values
    decided = (mx[:, 0] - below) > 2 * b_z.max(1).values
    t = z - mx
    ex = torch.exp(t)
    S = ex.sum(1, keepdim=True)
    lse = mx + torch.log(S)
    zy = z.gather(1, y.view(B, 1))
    loss = (lse - zy)[:, 0]
    rel_S = (ex * (E + 1) * U * (t.abs() + 1)).sum(1, keepdim=True) / S + g(K) + K * TINY / S
    b_lse = b_z.max(1, keepdim=True).values + rel_S + E * U * (S + 1) * torch.log(S).abs() + U * lse.abs()
    b_loss = (b_lse + b_z.gather(1, y.view(B, 1)))[:, 0] + U * loss.abs()
    ak = z - lse
    p = torch.exp(ak)
    onehot = F.one_hot(y, K).double()
    dl = (p - onehot) / B
    b_dl = (p * (b_z + b_lse + U * ak.abs() + E * U * (ak.abs() + 1)) + 3 * U * (p - onehot).abs()) / B + TINY
    gr = dl @ w / HW
    b_g = (b_dl @ w.abs() + g(K + 3) * (dl.abs() @ w.abs())) / HW
    b_g = b_g + half_ulp(gr.abs() + b_g, dtype)
    ref = dict(pooled=pooled, logits=z, loss=loss, dlogits=dl, dact=gr.view(B, 1, C).expand(B, HW, C).contiguous(),
               arg=arg, correct=int((arg == y).sum()), decided=decided)
    bound = dict(pooled=b_pooled, logits=b_z, loss=b_loss, dlogits=b_dl,
                 dact=b_g.view(B, 1, C).expand(B, HW, C).contiguous())
    return ref, bound


def head_sums_reference(dact_stored, act, y1, saved):
    """The BN-backward sums the fused head defines, from the gradient as stored: per slot row s the
    sums over the samples b = s (mod 8) and their pixels of dz = dact [act > 0] and dz (y1 - mean)
    invstd. (rows, bound), float64 [SLOTS, 2, C]."""
    B, HW, C = act.shape
    dz = dact_stored.double().view(B, HW, C) * (act.double() > 0)
    xh = (y1.double().view(B, HW, C) - saved[0].double()) * saved[1].double()
    terms = torch.stack([dz, dz * xh], 1)  # [B, 2, HW, C]
    rows = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    mag = torch.zeros(SLOTS, 2, C, dtype=torch.float64)
    for b in range(B):
        rows[b % SLOTS] += terms[b].sum(1)
        mag[b % SLOTS] += terms[b].abs().sum(1)
    return rows, g(HW + -(-B // SLOTS) + 4) * mag + TINY


def head_wgrad_reference(dlogits, pooled, gscale, sink=F32):
    """dw = gscale dlogits^T pooled, db = gscale sum_b dlogits: (dw, db, bound of dw, bound of db)."""
    gs = f32(gscale)
    dl, p = dlogits.double(), pooled.double()
    B = dl.shape[0]
    dw, db = gs * (dl.t() @ p), gs * dl.sum(0)
    b_dw = g(B + 2) * gs * (dl.abs().t() @ p.abs())
    b_db = g(B + 1) * gs * dl.abs().sum(0)
    return dw, db, b_dw + half_ulp(dw.abs() + b_dw, sink), b_db + half_ulp(db.abs() + b_db, sink)


# ---------------------------------------------------------------------------- fp32 evaluations
WRONG = ("bias_twice", "no_inv_hw", "tie_high", "slot0", "db_unscaled")


def head_fp32(inp, wrong=None):
    """The head's formulas in plain torch fp32 on the CPU (what a correct fp32 implementation
    computes), or one of the WRONG variants of them."""
    B, HW, C, K, dtype = (inp[k] for k in ("B", "HW", "C", "K", "dtype"))
    a, w, bias, y = inp["act"].float(), inp["w"], inp["bias"], inp["labels"].long()
    inv_hw = torch.tensor(1.0 if wrong == "no_inv_hw" else 1.0 / HW, dtype=F32)
    pooled = a.sum(1) * inv_hw
    z = pooled @ w.t() + bias
    if wrong == "bias_twice":
        z = z + bias
    mx = z.max(1, keepdim=True).values
    idx = torch.arange(K).expand(B, K)
    if wrong == "tie_high":
        arg = torch.where(z == mx, idx, torch.full_like(idx, -1)).max(1).values
    else:
        arg = torch.where(z == mx, idx, torch.full_like(idx, K)).min(1).values
    lse = mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True))
    loss = (lse - z.gather(1, y.view(B, 1)))[:, 0]
    dl = (torch.exp(z - lse) - F.one_hot(y, K).float()) * torch.tensor(1.0 / B, dtype=F32)
    gr = ((dl @ w) * inv_hw).to(dtype)
    return dict(pooled=pooled, logits=z, loss=loss, dlogits=dl, dact=gr.view(B, 1, C).expand(B, HW, C).contiguous(),
                correct=int((arg == y).sum()))


def sums_fp32(dact_stored, act, y1, saved, wrong=None):
    B, HW, C = act.shape
    d = dact_stored.float().view(B, HW, C)
    dz = torch.where(act.float() > 0, d, torch.zeros_like(d))
    x = dz * (y1.float().view(B, HW, C) - saved[0]) * saved[1]
    rows = torch.zeros(SLOTS, 2, C)
    for b in range(B):
        s = 0 if wrong == "slot0" else b % SLOTS
        rows[s, 0] += dz[b].sum(0)
        rows[s, 1] += x[b].sum(0)
    return rows


def wgrad_fp32(dl, pooled, gscale, sink, wrong=None):
    gs = torch.tensor(gscale, dtype=F32)
    dw = (dl.t() @ pooled) * gs
    db = dl.sum(0) * (1.0 if wrong == "db_unscaled" else gs)
    return dw.to(sink), db.to(sink)


HEAD_OUTPUTS = ("pooled", "logits", "loss", "dlogits", "dact")


def _all_cases():
    for shape in TABLE + (NULL_CASE,):
        for dtype in (F32, BF16):
            for kind in KINDS:
                yield head_inputs(*shape, dtype, kind)


def _what(inp):
    return tuple(inp[k] for k in ("B", "HW", "C", "K", "dtype", "kind"))


# ---------------------------------------------------------------------------- tests
def test_tables_reach_their_branches():
    """The thresholds of head_split / head_fused_ok / psx_head_wgrad at the table's shapes."""
    for B, HW, C, K in FUSED:
        assert not head_split(C, K) and head_fused_ok(C, K), (C, K)
    assert FUSED[4][3] * FUSED[4][2] == 1 << 18          # the last fused size
    assert max(K for _, _, _, K in FUSED) == 1024 and any(K > 256 for _, _, _, K in FUSED)  # 5th / 16th row trip
    assert {C for _, _, C, _ in FUSED} >= {16, 512, 1024}  # one short, one full, two pooling passes
    for B, HW, C, K in SPLIT:
        assert head_split(C, K), (C, K)
    assert not head_split(*NULL_CASE[2:], bufs=False) and head_split(*NULL_CASE[2:]) and head_fused_ok(*NULL_CASE[2:])
    for C, K in REFUSED:
        assert not head_split(C, K) and not head_fused_ok(C, K), (C, K)
    r = split_ranges(320, split_ks(320, False))           # ks 4, a short last range
    assert r == [(0, 96), (96, 192), (192, 288), (288, 320)]
    assert 841 % 4 == 1 and 841 % 32 and 33 % 32 == 1
    assert split_ks(1024, False) == 16 and split_ranges(1024, 16)[-1] == (960, 1024)
    r = split_ranges(64, split_ks(64, False))             # two of the four ranges empty
    assert [b >= e for b, e in r] == [False, False, True, True]
    assert 4104 > 1024 and not head_fused_ok(768, 400)
    assert split_ranges(320, split_ks(320, True)) == [(0, 320)]
    for B, K, C in WGRAD_SMALL:
        assert wgrad_small(K, C)
    for B, K, C in WGRAD_LARGE:
        assert not wgrad_small(K, C)
    assert {K % 4 for _, K, _ in WGRAD_SMALL} >= {1, 2} and any(C % 64 for _, _, C in WGRAD_SMALL)
    assert any(K % 8 for _, K, _ in WGRAD_LARGE) and any(C % 256 for _, _, C in WGRAD_LARGE)


def test_sums_ok_and_refusals_on_the_host():
    """psx_head_sums_ok against the mirrors, and the -2 refusals, which return before any launch."""
    from psx.ops import kernels as K
    from psx.ops._lib import kernels
    for _, _, C, nk in TABLE + (NULL_CASE,):
        assert K.head_sums_ok(C, nk) == (not head_split(C, nk) and head_fused_ok(C, nk)), (C, nk)
    for C, nk in REFUSED:
        assert not K.head_sums_ok(C, nk)
        for f32_ in (0, 1):
            assert kernels().psx_head_fwd_bwd(None, 2, 1, C, None, None, nk, None, None, None, None, None, None, None,
                                              f32_, None) == -2


def test_reference_equals_float64_autograd():
    for shape in TABLE:
        for kind in KINDS:
            inp = head_inputs(*shape, F32, kind)
            ref, _ = head_reference(inp)
            a = inp["act"].double().requires_grad_()
            w = inp["w"].double().requires_grad_()
            bias = inp["bias"].double().requires_grad_()
            z = F.linear(a.mean(1), w, bias)
            z.retain_grad()
            per = F.cross_entropy(z, inp["labels"].long(), reduction="none")
            per.mean().backward()
            for name, x in (("logits", z.detach()), ("loss", per.detach()), ("dlogits", z.grad), ("dact", a.grad)):
                scale = float(ref[name].abs().max()) + 1e-300
                assert float((x - ref[name]).abs().max()) <= 1e-12 * scale, (name, shape, kind)
            dw, db, _, _ = head_wgrad_reference(ref["dlogits"], ref["pooled"], 1.0)
            assert float((dw - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max()) + 1e-300, (shape, kind)
            assert float((db - bias.grad).abs().max()) <= 1e-12 * float(bias.grad.abs().max()) + 1e-300, (shape, kind)
            assert ref["correct"] == int((ref["logits"].argmax(1) == inp["labels"].long()).sum()) or kind == "tie"


def test_every_argmax_is_decided():
    """The exact ``correct`` count of the GPU tests rests on this."""
    for inp in _all_cases():
        ref, _ = head_reference(inp)
        assert bool(ref["decided"].all()), _what(inp)
        if inp["kind"] == "tie":
            T = tied_rows(inp["K"])
            assert bool((ref["arg"] == T[0]).all()), _what(inp)
            assert bool((ref["logits"][:, T] == inp["bias"][T[0]].double()).all())
            want = sum(1 for b in range(inp["B"]) if b % 3 == 0 or len(T) == 1)
            assert ref["correct"] == want, _what(inp)


def test_fp32_torch_stays_inside_every_bound():
    for inp in _all_cases():
        ref, bound = head_reference(inp)
        got = head_fp32(inp)
        for name in HEAD_OUTPUTS:
            assert_within(got[name], ref[name], bound[name], (name,) + _what(inp))
        assert got["correct"] == ref["correct"], _what(inp)
    for dtype in (F32, BF16):
        for shape in SUMS_CASES:
            inp = head_inputs(*shape, dtype, "plain")
            y1, saved = sums_inputs(shape[0], shape[1], shape[2], dtype)
            stored = head_fp32(inp)["dact"]
            rows, bound = head_sums_reference(stored, inp["act"], y1, saved)
            assert_within(sums_fp32(stored, inp["act"], y1, saved), rows, bound, ("sums", shape, dtype))
    for sink in (F32, F16):
        for gscale in GSCALES:
            for shape in WGRAD_SMALL + WGRAD_LARGE:
                dl, pooled = wgrad_inputs(*shape)
                dw, db, b_dw, b_db = head_wgrad_reference(dl, pooled, gscale, sink)
                gw, gb = wgrad_fp32(dl, pooled, gscale, sink)
                assert_within(gw, dw, b_dw, ("dw", shape, sink, gscale))
                assert_within(gb, db, b_db, ("db", shape, sink, gscale))


def _outside(x, ref, bound):
    return not bool(within(x, ref, bound).all())


def test_wrong_variants_leave_the_bounds():
    for shape in TABLE:
        B, HW, C, K = shape
        for dtype in (F32, BF16):
            inp = head_inputs(*shape, dtype, "plain")
            ref, bound = head_reference(inp)
            got = head_fp32(inp, "bias_twice")
            assert _outside(got["logits"], ref["logits"], bound["logits"]), shape
            if K > 1:  # one class: the loss is 0 and dlogits is 0 whatever the logit
                assert _outside(got["loss"], ref["loss"], bound["loss"]), shape
                assert _outside(got["dlogits"], ref["dlogits"], bound["dlogits"]), shape
            if HW > 1:
                got = head_fp32(inp, "no_inv_hw")
                assert _outside(got["pooled"], ref["pooled"], bound["pooled"]), shape
                if K > 1:
                    assert _outside(got["dact"], ref["dact"], bound["dact"]), shape
            if K >= 4:
                tie = head_inputs(*shape, dtype, "tie")
                assert head_fp32(tie, "tie_high")["correct"] != head_reference(tie)[0]["correct"], shape
    for dtype in (F32, BF16):
        for shape in SUMS_CASES:
            if shape[0] == 1:
                continue  # one sample: row 0 is its row
            inp = head_inputs(*shape, dtype, "plain")
            y1, saved = sums_inputs(shape[0], shape[1], shape[2], dtype)
            stored = head_fp32(inp)["dact"]
            rows, bound = head_sums_reference(stored, inp["act"], y1, saved)
            assert _outside(sums_fp32(stored, inp["act"], y1, saved, "slot0"), rows, bound), shape
    for sink in (F32, F16):
        for shape in WGRAD_SMALL + WGRAD_LARGE:
            dl, pooled = wgrad_inputs(*shape)
            dw, db, b_dw, b_db = head_wgrad_reference(dl, pooled, GSCALES[1], sink)
            gw, gb = wgrad_fp32(dl, pooled, GSCALES[1], sink, "db_unscaled")
            assert _outside(gb, db, b_db) and not _outside(gw, dw, b_dw), (shape, sink)


def test_half_ulp():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 65504.0, 2.0 ** -20, 0.0], dtype=torch.float64)
    assert half_ulp(v, BF16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** 7, 2.0 ** -28, 2.0 ** -134]
    assert half_ulp(v, F16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** 4, 2.0 ** -25,
                                         2.0 ** -25]
    assert not half_ulp(v, F32).any()
    x = torch.linspace(0.01, 3.0, 1001, dtype=torch.float64)
    assert bool(((x - x.to(BF16).double()).abs() <= half_ulp(x, BF16)).all())
    assert bool(((x - x.to(F16).double()).abs() <= half_ulp(x, F16)).all())
