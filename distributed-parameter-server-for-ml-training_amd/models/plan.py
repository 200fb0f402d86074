"""The step plan: which launches every layer of the worker step gets, decided once.

``plan_step(spec, batch, f32, opts)`` is a pure function of (network, batch, dtype, options): it
asks the kernel library's host-only queries (ops/kernels.py: wino_ok, conv2_path, ...), touches
no device and allocates nothing. models/engine.py allocates what the plan sizes and issues what it
routes; tests/test_engine_plan_cpu.py pins it against tests/golden/engine_plans.json.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

from ..ops import kernels as K
from ..utils.tune import tune, tune_flag
from .resnet import Bottleneck, BasicBlock

# fp32 Winograd F(4x4,3x3) forward and data gradient on images up to 64x64 (every 3x3 stride-1
# layer of ResNet-18 CIFAR and ResNet-50's 56x56 / 28x28 ones; R50 fp32 top-k 3,060 -> 3,188 img/s)
WINO_MAXHW = 64
# Winograd weight gradient up to 64x64 images: ResNet-50's 56x56 3x3 layers take the fused
# one (their direct alternative is wgrad2f: the tap-reuse kernel needs power-of-two rows):
# same box 36.8 -> 36.4 ms/step (profiles/r5_numbers.jsonl r5_call6)
WINO_WGRAD_MAXHW = 64
# fused weight gradient (wino_wgrad.hip) on images of at least 16x16: same box,
# B = 128, us incl. output transform, fused vs three-launch (profiles/r4_wino_wgrad_ab.jsonl,
# one row per layer): 32x32x64 58.4 vs 71.2, 16x16x128 55.3 vs 46.9 (+ the
# forward's V store the three-launch path needs, ~7), 8x8x256 53.7 vs 43.2, 4x4x512 61.7 vs
# 44.1. In the step (side stream; the forward's V store is on the critical path) same box:
# off 3.568, >= 32 3.412, >= 16 3.363-3.372 ms/step (profiles/r4_numbers.jsonl)
WINO_WGF_MINHW = 16


def _pow2_ceil(v: int, lo: int = 8) -> int:
    p = lo
    while p < v:
        p *= 2
    return p


@dataclass
class ConvSpec:
    name: str
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    h: int = 0  # input spatial
    w: int = 0
    need_dgrad: bool = True
    cp: int = 0
    kg: int = 0
    kgd: int = 0

    def finalize(self, chunk: int = 8):
        # input channels padded to a power of two >= one 16-byte chunk (8 bf16 / 4 fp32)
        self.cp = _pow2_ceil(self.cin, chunk)
        self.kg = -(-(self.k * self.k * self.cp) // 64) * 64
        self.kgd = self.k * self.k * self.cout  # cout % 64 == 0 for every ResNet conv
        assert self.kgd % 64 == 0 and self.cout % 64 == 0, self.name

    @property
    def out_hw(self):
        return K.conv_out_hw(self.h, self.w, self.k, self.stride, self.pad)


@dataclass
class BNSpec:
    name: str
    c: int


@dataclass
class BlockSpec:
    convs: list
    bns: list
    down: tuple | None = None  # (ConvSpec, BNSpec)


@dataclass
class NetSpec:
    stem_conv: ConvSpec
    stem_bn: BNSpec
    maxpool: bool
    blocks: list = field(default_factory=list)
    fc: str = "fc"
    fc_in: int = 512
    classes: int = 100
    in_hw: tuple = (32, 32)


def netspec_from_module(model, in_hw, f32: bool = False) -> NetSpec:
    """The network as the engine runs it; conv operands padded for the compute dtype (``f32``)."""
    def conv_of(m, name, h, w):
        cs = ConvSpec(name, m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], h, w)
        cs.finalize(4 if f32 else 8)
        return cs

    h, w = in_hw
    stem = conv_of(model.conv1, "conv1", h, w)
    stem.need_dgrad = False
    h, w = stem.out_hw
    maxpool = hasattr(model, "maxpool")
    if maxpool:
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    spec = NetSpec(stem, BNSpec("bn1", model.bn1.num_features), maxpool)
    for li in range(1, 5):
        layer = getattr(model, f"layer{li}")
        for bi, blk in enumerate(layer):
            pre = f"layer{li}.{bi}"
            if isinstance(blk, BasicBlock):
                names = ["conv1", "conv2"]
                down_mod = blk.shortcut if len(blk.shortcut) else None
                down_names = (f"{pre}.shortcut.0", f"{pre}.shortcut.1")
            elif isinstance(blk, Bottleneck):
                names = ["conv1", "conv2", "conv3"]
                down_mod = blk.downsample
                down_names = (f"{pre}.downsample.0", f"{pre}.downsample.1")
            else:
                raise TypeError(type(blk))
            convs, bns = [], []
            ch, cw = h, w
            for i, n in enumerate(names):
                m = getattr(blk, n)
                cs = conv_of(m, f"{pre}.{n}", ch, cw)
                convs.append(cs)
                bns.append(BNSpec(f"{pre}.bn{i + 1}", getattr(blk, f"bn{i + 1}").num_features))
                ch, cw = cs.out_hw
            down = None
            if down_mod is not None:
                ds = conv_of(down_mod[0], down_names[0], h, w)
                down = (ds, BNSpec(down_names[1], down_mod[1].num_features))
            spec.blocks.append(BlockSpec(convs, bns, down))
            h, w = ch, cw
    spec.fc_in = model.fc.in_features
    spec.classes = model.fc.out_features
    spec.in_hw = tuple(in_hw)
    return spec


def all_convs(spec: NetSpec):
    yield spec.stem_conv
    for b in spec.blocks:
        yield from b.convs
        if b.down:
            yield b.down[0]


def all_bns(spec: NetSpec):
    yield spec.stem_bn
    for b in spec.blocks:
        yield from b.bns
        if b.down:
            yield b.down[1]


@dataclass(frozen=True)
class EngineOptions:
    """What an engine is built with; fixed for its life. ``from_env`` is the one reader of
    PSX_TUNE / PSX_DETERMINISTIC; every default is the measured-best path."""
    # every BN statistic accumulates as exact fixed-point integers (csrc/kernels/bnfin.hpp DetRed),
    # so two runs of a step give bit-identical gradients, for +0-2 % step time
    deterministic: bool = True
    # where the training-mode BN finalize runs. "apply": folded into the consuming apply launches
    # (bnfin.hpp bn_fin_lds): every apply workgroup re-derives the affine/coefficients from the
    # stat slots, removing 40 finalize launches per step. With 32 slot rows it measured slower
    # (2.18 vs 2.10 ms/step); with 8 rows (csrc/kernels/common.hpp) it wins: 1.999 vs 2.019
    # ms/step. "conv": inside the producing launch (last workgroup). "separate": launches of its own.
    bn_finalize: str = "apply"
    # BN-backward sums from the dgrad epilogue (skips the separate bn_bwd_reduce pass where a
    # dgrad produces the BN's input gradient): neutral with 32 stat slots + separate finalize
    # (2.215 vs 2.217 ms/step), a small win with 8 slots + folded finalize (1.996/2.000 vs
    # 2.010/2.006 ms/step, two same-box A/B pairs). With it the dgrad epilogue already reads the
    # ReLU mask operand o: it stores dz = g*[o > 0] instead of g (bwd_stats_desc mask_store), the
    # BN-backward apply then runs without o (one activation read less per BN layer) and dz doubles
    # as the identity shortcut's gradient (no dzout copy)
    fuse_bnbwd: bool = True
    # BN-backward applies folded into the consuming Winograd data gradient + dy transform: "all",
    # "dz_only" (only the three-launch layers' one pass over dz), "off" (PSX_TUNE wino_bwdfold=0)
    bwd_fold: str = "all"
    # the stride-2 block's 1x1 shortcut data gradient folded into the 3x3 one's launch
    fold_sc: bool = True
    # the direct stem kernels (csrc/kernels/stem.hip) where they exist: fp32 (CIFAR 3x3: 27.4 ->
    # 19.5 us in isolation, bench/stem_probe.py; step A/B within noise, bf16 unmeasured in
    # isolation; and ImageNet 7x7) and the bf16 ImageNet 7x7
    stem_direct: bool = True
    # weight gradients (+ their batched reductions) on a side stream, a parallel branch of the
    # captured step graph next to the dgrad -> BN-backward chain. PSX_TUNE wgrad_stream=1 / 0
    # forces it; None (auto) keeps it except for the fp32 engine on CIFAR-size images, whose
    # fused Winograd weight gradients (1 workgroup per CU, like the data gradients beside them)
    # only time-share the chip with the dgrad chain and add cross-queue waits: same box
    # 3.35-3.38 -> 3.28-3.29 ms/step without it (r4_call20/21); bf16 ResNet-18 (1.85 -> 1.89)
    # and fp32 ResNet-50 (40.4 -> 41.5) keep it.
    wgrad_stream: bool | None = None
    wino: bool = True          # PSX_TUNE wino=0: direct kernels everywhere
    wino_bnfold: bool = True   # PSX_TUNE wino_bnfold=0: BN + ReLU not folded into the next Winograd conv
    wgrad_rbatch: bool = True  # PSX_TUNE wgrad_rbatch=0: per-layer weight-gradient reductions

    def __post_init__(self):
        assert self.bn_finalize in ("apply", "conv", "separate"), self.bn_finalize
        assert self.bwd_fold in ("all", "dz_only", "off"), self.bwd_fold

    @classmethod
    def from_env(cls, f32: bool, in_hw, deterministic=None) -> "EngineOptions":
        if deterministic is None:
            deterministic = os.environ.get("PSX_DETERMINISTIC", "1") == "1"
        ws = tune("wgrad_stream", "auto")
        if ws == "auto":
            ws = "0" if (f32 and max(in_hw) <= 64) else "1"
        return cls(deterministic=bool(deterministic), wgrad_stream=ws == "1", wino=tune_flag("wino", True),
                   bwd_fold="all" if tune_flag("wino_bwdfold", True) else "off",
                   wino_bnfold=tune_flag("wino_bnfold", True), wgrad_rbatch=tune_flag("wgrad_rbatch", True))


@dataclass
class ConvPlan:
    wf_off: int            # forward operand rows in wbuf; data-gradient rows at wd_off (-1: none)
    wd_off: int
    splits: int            # direct weight gradient: split-K partials [splits][cout][kg] at wp_off of wpart_w
    wp: int
    wp_off: int = 0
    fwd: str = "conv2"     # stem | conv2 | wino3 | wino_fused
    dgrad: str | None = "conv2"  # conv2 | conv2_sc | wino3 | wino_pre | wino_fused | None (no launch of its own)
    wgrad: str = "wgrad2"  # wgrad2 | wino3 | wino_dz | wino_fused
    uf_rows: int = 0       # Winograd: rows per (cout, cin) of U / U' (36, or 40 for the fused kernel)
    ud_rows: int = 0
    v_floats: int = 0      # > 0: the forward keeps its transformed input V for the weight gradient
    rbatch: bool = False   # its reduce joins the block's one wgrad_reduce_batch launch
    late: bool = False     # its weight transform runs late, on the side stream
    xfold: bool = False    # its input relu(BN(y)) is never written (applied by its input transform)
    tail: bool = False     # the step's tail weight gradient (compute stream, own scratch)
    bwd_fold: bool = False  # its gradients read dz: the BN-backward apply in front of it is folded in

    @property
    def wino(self) -> bool:
        return self.fwd.startswith("wino")

    @property
    def keep_v(self) -> bool:
        return self.v_floats > 0


@dataclass
class BnPlan:
    fwd_off: int           # slot rows in the slot buffer: forward [2][C], backward [3][C]
    bwd_off: int
    ctr: int               # its two finalize counters (forward, backward)
    shift_off: int
    fwd_fin: str = "apply"   # apply | conv | separate | next_conv (the next conv's input transform)
    bwd_sums: str | None = "reduce"  # reduce | dgrad | head; None: with its block's output BN (a pair)
    premasked: bool | None = False   # the incoming gradient is dz = g*[o > 0] already
    bwd_apply: str = "pass"  # pass | folded (into the consuming conv's gradients) | pair


@dataclass
class StepPlan:
    opts: EngineOptions
    batch: int
    f32: bool
    wgrad_stream: bool
    nslots: int            # PSX_STAT_SLOTS slot rows per BN statistic
    slot_words: int        # floats per statistic and channel: nslots (x det_slot_scale, deterministic)
    convs: dict = field(default_factory=dict)
    bns: dict = field(default_factory=dict)
    bnfold: dict = field(default_factory=dict)  # BN -> the conv whose input transform applies it
    wbuf: int = 0
    wpart: int = 0         # conv split-K slabs (compute stream)
    wpart_w: int = 0       # weight-gradient partials (own buffer: may run on the side stream)
    s_main: int = 0        # Winograd scratch: compute stream (two of these), dy tiles, GEMM partials
    s_d: int = 0
    s_part: int = 0
    red_len: int = 0
    ctr_words: int = 0
    nshift: int = 0
    tail_split: bool = False

    def wino_names(self):
        return [n for n, p in self.convs.items() if p.wino]

    def dz_names(self):
        return [n for n, p in self.convs.items() if p.wgrad == "wino_dz"]

    def late_names(self):
        return [n for n, p in self.convs.items() if p.late]

    def bwd_fold_names(self):
        return [n for n, p in self.convs.items() if p.bwd_fold]


def _plan_wino(spec, B, side, convs):
    """fp32 Winograd F(4x4,3x3) (csrc/kernels/wino.hip) for the 3x3 / stride-1 layers: forward
    and data gradient on images up to WINO_MAXHW, weight gradient up to WINO_WGRAD_MAXHW
    (on 32x32 the direct tap-reuse kernel is faster than the three-launch one, 101 vs 129 us).
    Same-box per-layer A/B in profiles/r2s4_wino_*.jsonl. Per layer: the transformed forward weights
    U [cout][36][cin] and data-gradient weights U' [cin][36][cout] (rebuilt by unpack() every
    step) and, where the weight gradient is Winograd, the transformed input V [36][T][cin] the
    forward leaves for it. In deterministic mode its BN sums take the fixed-order reduction
    like every other producer (wino_out_kernel + bnfin.hpp DetRed). Not for bf16.
    Layers with 64 / 128 input channels (ResNet-18's 32x32 and 16x16
    stages) run forward and data gradient as ONE fused launch each (wino_fused.hip: the
    transforms inside the GEMM, V / P never in HBM; the other layers take the three-launch path;
    bench/wino_fused_ab.py: 32x32x64 fwd / dgrad 80 / 95 -> 58 / 63 us, 16x16x128 59 / 62 -> 50 / 51).
    The fused forward still writes V where the Winograd weight gradient reads it.
    Returns the scratch sizes (s_main, s_d, s_part)."""
    s_main = s_d = s_part = 0
    for cs in all_convs(spec):
        if (cs.k != 3 or cs.stride != 1 or cs.pad != 1 or cs.cp != cs.cin or cs.h > WINO_MAXHW or cs.w > WINO_MAXHW
                or not K.wino_ok(cs.h, cs.w, cs.cp, cs.cout)):
            continue
        p = convs[cs.name]
        vk, vc = K.wino_v_floats(B, cs.h, cs.w, cs.cout), K.wino_v_floats(B, cs.h, cs.w, cs.cp)
        s_main = max(s_main, vk, vc, K.wino_p_floats(B, cs.h, cs.w, cs.cp, cs.cout),
                     K.wino_p_floats(B, cs.h, cs.w, cs.cout, cs.cp))
        # fused single-launch kernel (wino_fused.hip) where it applies, per direction
        ff = K.wino_fused_ok(B, cs.h, cs.w, cs.cp, cs.cout)
        fd = cs.need_dgrad and K.wino_fused_ok(B, cs.h, cs.w, cs.cout, cs.cp)
        p.fwd, p.uf_rows = ("wino_fused", 40) if ff else ("wino3", 36)
        if cs.need_dgrad:
            p.dgrad, p.ud_rows = ("wino_fused", 40) if fd else ("wino3", 36)
        q = K.wino_wgrad_q(B, cs.h, cs.w, cs.cp, cs.cout) if max(cs.h, cs.w) <= WINO_WGRAD_MAXHW else 0
        if q <= 0:
            continue  # direct weight gradient; the forward's V goes to scratch
        # fused weight gradient (wino_wgrad.hip): transforms x and dy itself, so the forward keeps
        # no V and no D is formed
        qf = K.wino_wgrad_fused_q(B, cs.h, cs.w, cs.cp, cs.cout) if min(cs.h, cs.w) >= WINO_WGF_MINHW else 0
        if qf:
            p.wgrad = "wino_fused"
            s_part = max(s_part, 36 * qf * cs.cout * cs.cp)
            continue
        p.wgrad, p.v_floats = "wino3", vc
        s_d = max(s_d, vk)
        s_part = max(s_part, 36 * q * cs.cout * cs.cp)
        # one pass over dz forms both backward operands (wino.hip wino_dz_xf_kernel): D for the
        # weight gradient and V' for the data gradient, instead of a dy transform and an input
        # transform that each read dy. Only with both gradients on the compute stream: on the side
        # stream D would be written into scratch that stream still reads.
        if not side and cs.need_dgrad and not fd and K.wino_dz_ok(B, cs.h, cs.w, cs.cout):
            p.wgrad, p.dgrad = "wino_dz", "wino_pre"
    return s_main, s_d, s_part


def _sc_folds(cs: ConvSpec, ds: ConvSpec, B, f32) -> bool:
    """The block's 1x1 / stride-2 shortcut data gradient folds into the 3x3 / stride-2 one's launch."""
    if cs.k != 3 or cs.stride != 2 or cs.pad != 1 or ds.k != 1 or ds.stride != 2 or ds.pad != 0 \
            or ds.cp != cs.cp or ds.cout != cs.cout or ds.kgd != cs.cout:
        return False
    return K.conv2_path("dgrad_sc", B, cs.h, cs.w, cs.cp, cs.cout, cs.k, cs.stride, cs.pad, cs.kgd, f32) != -11


def plan_step(spec: NetSpec, batch: int, f32: bool, opts: EngineOptions) -> StepPlan:
    B = batch
    side = opts.wgrad_stream if opts.wgrad_stream is not None else not (f32 and max(spec.in_hw) <= 64)
    fold = opts.bn_finalize == "apply"
    # deterministic mode: every slot entry is a 16-byte fixed-point pair (bnfin.hpp DetRed)
    nslots = K.bn_bwd_reduce_T(1, 64)
    plan = StepPlan(opts, B, f32, side, nslots, nslots * (K.det_slot_scale() if opts.deterministic else 1))
    convs, bns = plan.convs, plan.bns

    # operands: one buffer holding every conv's forward (and data-gradient) rows; fp32 scratch:
    # weight-gradient split-K partials and conv split-K slabs (stream-ordered on the compute stream)
    max_wp = 0
    for cs in all_convs(spec):
        wf_off, wd_off = plan.wbuf, -1
        plan.wbuf += cs.cout * cs.kg
        if cs.need_dgrad:
            wd_off = plan.wbuf
            plan.wbuf += cs.cp * cs.kgd
        s = K.conv_wgrad2_splits(B, cs.h, cs.w, cs.cp, cs.cout, cs.k, cs.stride, cs.pad, cs.kg, f32)
        p = convs[cs.name] = ConvPlan(wf_off, wd_off, s, s * cs.cout * cs.kg, dgrad="conv2" if cs.need_dgrad else None)
        max_wp = max(max_wp, p.wp)
        oh, ow = cs.out_hw
        plan.wpart = max(plan.wpart, K.conv2_workspace_bytes(B, oh, ow, cs.cout, cs.kg, f32) // 4,
                         K.conv2_workspace_bytes(B, cs.h, cs.w, cs.cp, cs.kgd, f32) // 4 if cs.need_dgrad else 0)
        if (opts.stem_direct and (f32 or cs.k == 7) and opts.bn_finalize != "conv" and cs.cin == 3
                and (cs.k, cs.stride, cs.pad) in ((3, 1, 1), (7, 2, 3))
                and K.stem_ok(B, cs.h, cs.w, cs.cin, cs.cp, cs.cout, cs.kg, f32, k=cs.k)):
            p.fwd = "stem"
    if f32 and opts.wino:
        plan.s_main, plan.s_d, plan.s_part = _plan_wino(spec, B, side, convs)
    # Batched weight-gradient reduction: the layers of one residual block keep their split-K
    # partials in disjoint slices of wpart_w until ONE wgrad_reduce_batch launch at the end of the
    # block's backward reduces them all (8 launches instead of 19 for ResNet-18)
    plan.wpart_w = max_wp
    for b in spec.blocks:
        bc = list(b.convs) + ([b.down[0]] if b.down else [])
        if not opts.wgrad_rbatch or len(bc) > K.WRBATCH_MAX:
            continue
        off = 0
        for cs in bc:
            p = convs[cs.name]
            p.wp_off = off
            off += p.wp
            p.rbatch = p.wgrad == "wgrad2" and K.wgrad_reduce_batchable(cs.cp, cs.k)
        plan.wpart_w = max(plan.wpart_w, off)
    # the later stages' Winograd weight transforms overlap the first stage's forward on the side
    # stream; without one they stay on the compute stream (a stream of their own measured 3.36 vs
    # 3.28 ms/step: a forked branch at the step start costs more than the overlap returns,
    # r4_numbers.jsonl r4_call23)
    hw0 = max((cs.h for cs in all_convs(spec) if convs[cs.name].wino), default=0)
    for cs in all_convs(spec):
        convs[cs.name].late = side and convs[cs.name].wino and cs.h != hw0
    # the first block's first conv's Winograd weight gradient runs on the compute stream after the
    # stem's BN backward, concurrently with the side stream's: its own scratch
    if side and spec.blocks and convs[spec.blocks[0].convs[0].name].wgrad != "wgrad2":
        plan.tail_split = convs[spec.blocks[0].convs[0].name].tail = True

    # BN slots: the first ctr_words of the slot buffer are the in-launch finalize counters (two
    # per BN layer: forward, backward; csrc/kernels/bnfin.hpp), zeroed with the slots every step
    plan.ctr_words = -(-2 * len(list(all_bns(spec))) // 64) * 64
    off = plan.ctr_words
    for i, (cs, bs) in enumerate(zip(all_convs(spec), all_bns(spec))):  # each conv and the BN behind it
        bwd = off + plan.slot_words * 2 * bs.c
        # no in-launch finalize on the Winograd path
        fin = "separate" if opts.bn_finalize == "conv" and convs[cs.name].wino else opts.bn_finalize
        bns[bs.name] = BnPlan(off, bwd, 2 * i, plan.nshift, fwd_fin=fin)
        off = bwd + plan.slot_words * 3 * bs.c
        plan.nshift += bs.c
    plan.red_len = off
    # BN folded into the next conv's input transform: a block's inner BN (+ ReLU) whose only
    # consumer is a Winograd conv with a Winograd weight gradient (that reads V, not the
    # activation) is finalized and applied inside wino_in_kernel, so its activation is never
    # written; the data gradient's ReLU mask comes from the BN affine (needs the masked dz store,
    # so the BN-backward apply never reads the activation either)
    if fold and opts.fuse_bnbwd and opts.wino_bnfold:
        for b in spec.blocks:
            for i in range(len(b.convs) - 1):
                nxt = b.convs[i + 1]
                if convs[nxt.name].wgrad != "wgrad2" and nxt.cin == b.bns[i].c:
                    plan.bnfold[b.bns[i].name] = nxt.name
                    bns[b.bns[i].name].fwd_fin = "next_conv"
                    convs[nxt.name].xfold = True

    # backward: who produces each BN's sums, and whether its apply is a pass of its own
    def into(bs: BNSpec, cs: ConvSpec | None = None):
        """bs's input gradient comes out of a dgrad; cs: the one conv whose gradients consume bs's."""
        bp, cp = bns[bs.name], convs[cs.name] if cs is not None else None
        if opts.fuse_bnbwd:
            bp.bwd_sums, bp.premasked = "dgrad", True
        # Folded: cs has the fused Winograd data gradient (or the one pass over dz) and a Winograd
        # weight gradient, g is already the masked dz and its sums came from the producing dgrad
        if (cp is not None and opts.bwd_fold != "off" and fold and bp.premasked and cp.wgrad != "wgrad2"
                and (cp.dgrad == "wino_fused" and opts.bwd_fold == "all" or cp.wgrad == "wino_dz")):
            bp.bwd_apply, cp.bwd_fold = "folded", True

    for j, b in enumerate(spec.blocks):
        for i in range(len(b.convs) - 1):
            into(b.bns[i], b.convs[i])
        nxt = j + 1 < len(spec.blocks)
        if b.down:
            bns[b.down[1].name].bwd_sums = bns[b.down[1].name].premasked = None
            bns[b.down[1].name].bwd_apply = "pair"
            if nxt:
                into(b.bns[-1])
            cs, ds = b.convs[0], b.down[0]
            if opts.fold_sc and not convs[cs.name].wino and _sc_folds(cs, ds, B, f32):
                convs[cs.name].dgrad, convs[ds.name].dgrad = "conv2_sc", None
        elif nxt:
            into(b.bns[-1], b.convs[-1])
        elif opts.fuse_bnbwd and K.head_sums_ok(spec.fc_in, spec.classes):
            # the last block's output BN: its backward sums come out of the head launch (one
            # bn_bwd_reduce pass fewer) when the fused per-sample head runs and that BN has no
            # shortcut BN sharing its gradient
            bns[b.bns[-1].name].bwd_sums = "head"
    if spec.blocks and not spec.maxpool:  # not across the ResNet-50 max-pool
        into(spec.stem_bn)
    return plan
