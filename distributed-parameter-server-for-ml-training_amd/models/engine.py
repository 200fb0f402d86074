"""HIP training engine: ResNet forward/backward on hand-written CDNA4 kernels.

This is the MI355X replacement for the worker's ``train_local_batch`` (reference:
src/workers/worker.py:333-348 — zero_grad, forward, CrossEntropyLoss, backward) and for
``evaluate_model`` (worker.py:313-331). Instead of autograd over ``nn.Module``s it runs an
explicit, statically-scheduled forward + backward over pre-allocated HBM buffers:

* activations NHWC in the compute dtype — bf16 (fast path) or fp32 (``dtype=torch.float32``,
  the reference's training precision, worker.py:333-348: conv operands and activations fp32,
  every product on the exact-f32 MFMA ``v_mfma_f32_16x16x4_f32``); conv = MFMA implicit GEMM
  (fwd / dgrad / split-K wgrad), BN batch statistics produced by the conv epilogue,
  BN+ReLU(+residual) fused elementwise passes, fused pool+FC+softmax-xent head;
* gradients are written straight into one flat wire buffer (fp16 codec by default) laid out
  like the trainable-parameter prefix of the parameter arena (models/layout.py), so a push is
  a single RCCL reduce/send of one buffer and the server update one fused kernel;
* parameters are read from a worker-local fp32 arena (the fetched server state) and unpacked
  to implicit-GEMM operands of the compute dtype by one table-driven kernel per fetch;
* no allocation, host sync or data-dependent host control flow inside a step, so the whole
  step (unpack + augment + fwd + bwd) is captured once into a HIP graph and replayed.

The network is described by a generic block list so ResNet-18 (CIFAR stem) and ResNet-50
(ImageNet stem with max-pool) share one engine.
"""
from __future__ import annotations

import contextlib
from dataclasses import replace

import numpy as np
import torch

from ..ops import kernels as K
from .layout import ParamLayout
from .plan import BNSpec, ConvSpec, EngineOptions, all_bns, all_convs, netspec_from_module, plan_step

CIFAR_MEAN = (0.5071, 0.4867, 0.4408)  # reference worker.py:149-150
CIFAR_STD = (0.2675, 0.2565, 0.2761)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_BN_PARAMS = ("weight", "bias", "running_mean", "running_var")


class HipResNetEngine:
    """Pre-allocated, graph-capturable ResNet training step on psx HIP kernels."""

    def __init__(self, model: torch.nn.Module, layout: ParamLayout, batch: int, device="cuda",
                 grad_dtype=torch.float16, in_hw=(32, 32), mean=CIFAR_MEAN, std=CIFAR_STD, bn_eps=1e-5,
                 bn_momentum=0.1, seed=1234, dtype=torch.bfloat16, deterministic=None,
                 options: EngineOptions | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("HipResNetEngine needs an MI355X (torch.cuda / HIP device)")
        K.unpack_desc_size()  # fail loudly right here if the native library is missing
        self.dev = torch.device(device)
        self.layout = layout
        self.B = batch
        self.grad_dtype = grad_dtype
        self.grad_fp16 = grad_dtype == torch.float16
        # compute dtype of activations and conv operands (fp32 = the reference's precision)
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"engine dtype {dtype}: bfloat16 or float32")
        self.dtype = dtype
        self.f32 = dtype == torch.float32
        self.spec = netspec_from_module(model, in_hw, self.f32)
        # the options (models/plan.py EngineOptions; default: PSX_TUNE / PSX_DETERMINISTIC) and the
        # step plan made from them are fixed for the engine's life
        if options is None:
            options = EngineOptions.from_env(self.f32, in_hw, deterministic)
        elif deterministic is not None:
            options = replace(options, deterministic=bool(deterministic))
        self.opts = options
        self.deterministic = options.deterministic
        self.plan = plan_step(self.spec, batch, self.f32, options)
        self.mean, self.std = mean, std
        self.eps, self.mom = bn_eps, bn_momentum
        self.seed = seed
        self.graph = None
        self.graphs = None
        self.segments = None  # backward split points (set_segments), None = one segment
        # the side stream of the weight gradients and the late Winograd weight transforms
        self.wg_stream = torch.cuda.Stream(device=self.dev) if self.plan.wgrad_stream else None
        self._wg_batch = self._wr_batch = None  # issue queues of one backward unit (_bwd_block)
        self._late_ev = None
        self._wino_wb_key = None
        self._zeroed = False       # red zeroed by this step's augment launch (consumed by forward)
        self._zeroed_head = False  # correct zeroed by it (consumed by head)
        self._fins = {}
        self.wsrc = None        # bf16 weight image to unpack from (set_weight_source), None = arena
        self.pre_unpack = None
        self.small_scatter = None
        self._build()

    def _set_unpack_descs(self, convs):
        """The param_unpack_tiles table: one descriptor per conv whose implicit-GEMM operands
        (forward rows at wf_off, data-gradient rows at wd_off of wbuf) are unpacked each step."""
        descs = []
        tile0 = 0  # flat grid of param_unpack_tiles: (64x64 (oc, c) tile, chunk of <= 3 taps) units
        for cs in convs:
            p = self.plan.convs[cs.name]
            descs.append((self.layout.offset(f"{cs.name}.weight"), p.wf_off, p.wd_off, cs.cout, cs.cin, cs.k, cs.k,
                          cs.cp, cs.kg, cs.kgd, tile0))
            tile0 += -(-cs.cout // 64) * -(-cs.cp // 64) * -(-(cs.k * cs.k) // 3)
        self.ntiles = tile0
        dsz = K.unpack_desc_size()
        assert dsz == 3 * 8 + 8 * 4, dsz
        raw = np.zeros(len(descs), dtype=np.dtype([("o", "<i8", 3), ("i", "<i4", 8)]))
        for j, d in enumerate(descs):
            raw[j]["o"] = d[:3]
            raw[j]["i"] = d[3:]
        self.descs = torch.from_numpy(raw.view(np.uint8).copy()).to(self.dev)
        self.ndesc = len(descs)

    # ------------------------------------------------------------------ allocation
    def _bf(self, *shape):
        """An activation buffer of the compute dtype."""
        return torch.empty(*shape, dtype=self.dtype, device=self.dev)

    def _f32(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.dev)

    def _build(self):
        sp, B, plan = self.spec, self.B, self.plan
        # weights: one buffer of the compute dtype holding every conv's fwd (and dgrad) operand.
        # Winograd layers read their own transformed weights (unpack -> _wino_unpack): they are not
        # in the implicit-GEMM operand unpack (13 of ResNet-18's 20 convs, most bytes)
        self.wbuf = torch.zeros(plan.wbuf, dtype=self.dtype, device=self.dev)
        self._set_unpack_descs([cs for cs in all_convs(sp) if not plan.convs[cs.name].wino])

        H, W = sp.in_hw
        self.x0 = self._bf(B, H, W, sp.stem_conv.cp)
        self.labels = torch.zeros(B, dtype=torch.int32, device=self.dev)
        # [sample indices of the batch | step counter]: one host->device copy per step
        self.batch_meta = torch.zeros(B + 1, dtype=torch.int32, device=self.dev)
        self.index = self.batch_meta[:B]
        self.step_dev = self.batch_meta[B:]

        # Cross-workgroup reductions (BN fwd statistics from the conv epilogue, BN bwd sums) use
        # fp32 atomics into PSX_STAT_SLOTS slot rows per BN layer; all slot rows live in one
        # buffer that is zeroed once at the start of every step (one memset node in the graph).
        self.nslots = plan.nslots
        self.red = self._f32(plan.red_len)
        # BN statistic shifts (csrc/kernels/bnfin.hpp BnFin::sshift): the forward statistics are
        # sums of (y - k) and (y - k)^2 with k = the layer's previous batch mean, so the variance
        # never cancels two large numbers when |mean| >> std. Row 0 = this step's k (read-only
        # during the step), row 1 = the batch means the finalizes write; the next training step's
        # augment launch copies row 1 -> row 0. Zero at the first step (plain sums).
        self.bn_shift = torch.zeros(2, plan.nshift, dtype=torch.float32, device=self.dev)
        # per-BN persistent state: affine [2,C] (scale, shift), saved [2,C] (mean, invstd), coef [3,C]
        self.bn = {}
        for bs in all_bns(sp):
            so = plan.bns[bs.name].shift_off
            self.bn[bs.name] = dict(affine=self._f32(2, bs.c), saved=self._f32(2, bs.c), coef=self._f32(3, bs.c),
                                    c=bs.c, sshift=self.bn_shift[0, so:so + bs.c],
                                    sshift_next=self.bn_shift[1, so:so + bs.c])

        # activation / gradient buffers
        st = sp.stem_conv
        p, q = st.out_hw
        self.y0 = self._bf(B, p, q, st.cout)
        self.a0 = self._bf(B, p, q, st.cout)
        self.g0 = self._bf(B, p, q, st.cout)   # grad wrt a0 (or wrt maxpool input)
        self.dy0 = self._bf(B, p, q, st.cout)
        h_in = self.a0
        if sp.maxpool:  # ImageNet stem: 3x3/s2 max-pool after bn1+relu (csrc/kernels/pool.hip)
            mh, mw = (p + 2 - 3) // 2 + 1, (q + 2 - 3) // 2 + 1
            self.p0 = self._bf(B, mh, mw, st.cout)
            self.pidx = torch.empty(B, mh, mw, st.cout, dtype=torch.uint8, device=self.dev)
            h_in = self.p0
        self.blk = []
        self.xsrc = {}  # conv whose input relu(BN(y)) is never written -> (pre-BN y, BN affine)
        for b in sp.blocks:
            d = dict(inp=h_in)
            d["y"] = [self._bf(B, *cs.out_hw, cs.cout) for cs in b.convs]
            d["a"] = [self._bf(B, *cs.out_hw, cs.cout) for cs in b.convs[:-1]]
            d["dy"] = [self._bf(B, *cs.out_hw, cs.cout) for cs in b.convs]
            d["da"] = [self._bf(B, *cs.out_hw, cs.cout) for cs in b.convs[:-1]]
            last = b.convs[-1]
            d["out"] = self._bf(B, *last.out_hw, last.cout)
            d["gin"] = torch.empty_like(h_in)  # grad wrt block input
            for i, cs in enumerate(b.convs):
                if plan.convs[cs.name].xfold:
                    self.xsrc[cs.name] = (d["y"][i - 1], self.bn[b.bns[i - 1].name]["affine"])
            if b.down:
                ds, dbn = b.down
                d["ys"] = self._bf(B, *ds.out_hw, ds.cout)
                d["dys"] = self._bf(B, *ds.out_hw, ds.cout)
                d["dxs"] = torch.empty_like(h_in)
            else:
                d["dz"] = self._bf(B, *last.out_hw, last.cout)
            self.blk.append(d)
            h_in = d["out"]
        self.final = h_in
        # fp32 scratch: conv split-K slabs (stream-ordered on the compute stream) and the weight
        # gradients' split-K partials (own buffer: they may run on the side stream)
        self.wpart = self._f32(max(1, plan.wpart))
        self.wpart_w = self._f32(max(1, plan.wpart_w))
        # Winograd: per layer (U, U', V | None: the forward's V goes to scratch); compute-stream
        # scratch (forward V of layers without a Winograd weight gradient / GEMM output;
        # data-gradient input tiles + GEMM output) and the weight gradients' own (dy tiles, GEMM
        # partials), once more for the tail weight gradient that runs beside the side stream's
        self.wu = {}
        for cs in all_convs(sp):
            cp = plan.convs[cs.name]
            if cp.wino:
                self.wu[cs.name] = (self._f32(cp.uf_rows * cs.cout * cs.cp),
                                    self._f32(cp.ud_rows * cs.cout * cs.cp) if cp.ud_rows else None,
                                    self._f32(cp.v_floats) if cp.keep_v else None)
        if self.wu:
            self.wino_s1 = self._f32(max(1, plan.s_main))
            self.wino_s2 = self._f32(max(1, plan.s_main))
            self.wino_wd = self._f32(max(1, plan.s_d))
            self.wino_wpart = self._f32(max(1, plan.s_part))
            self.wino_tail = (self._f32(max(1, plan.s_d)), self._f32(max(1, plan.s_part))) if plan.tail_split else None
        # head
        fh, fw = self.final.shape[1], self.final.shape[2]
        self.head_hw = fh * fw
        self.pooled = self._f32(B, sp.fc_in)
        self.dlogits = self._f32(B, sp.classes)
        self.loss = self._f32(B)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.dfinal = torch.empty_like(self.final)
        # gradient wire buffer (trainable-parameter prefix of the arena)
        self.grads = torch.zeros(self.layout.param_numel, dtype=self.grad_dtype, device=self.dev)

    def _wino_unpack(self, arena):
        """Every Winograd layer's forward and data-gradient weight transforms: the first stage's
        layers in one launch on the compute stream, the rest (ResNet-18: 9.3 M of the 9.4 M
        Winograd weights, ~280 MB of transformed operands, ~80 us) in one launch on the side
        stream, overlapped with the forward of the first stage; the compute stream waits for it
        before the first conv that reads one of them (``_wino_late_wait``)."""
        key = arena.data_ptr()
        if self._wino_wb_key != key:
            early, late = [], []
            for cs in all_convs(self.spec):
                if cs.name not in self.wu:
                    continue
                p, (uf, ud, _) = self.plan.convs[cs.name], self.wu[cs.name]
                w = self._aview(arena, f"{cs.name}.weight")
                dst = late if p.late else early
                dst.append((w, uf, cs.cout, cs.cp, False, int(p.fwd == "wino_fused")))
                if ud is not None:
                    dst.append((w, ud, cs.cout, cs.cp, True, int(p.dgrad == "wino_fused")))
            self._wino_wb = K.WinoWeightBatch(early) if early else None
            self._wino_wb_late = K.WinoWeightBatch(late) if late else None
            self._wino_wb_key = key
        if self._wino_wb is not None:
            self._wino_wb()
        self._late_ev = None
        if self._wino_wb_late is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            self.wg_stream.wait_event(ev)
            with torch.cuda.stream(self.wg_stream):
                self._wino_wb_late()
                self._late_ev = torch.cuda.Event()
                self._late_ev.record(self.wg_stream)

    def _wino_late_wait(self, p):
        """The compute stream waits (once per step) for the side-stream weight transforms before
        the first conv that reads one of them."""
        if self._late_ev is not None and p.late:
            torch.cuda.current_stream(self.dev).wait_event(self._late_ev)
            self._late_ev = None

    # ------------------------------------------------------------------ helpers
    def _gptr(self, name: str) -> int:
        return self.grads.data_ptr() + self.grads.element_size() * self.layout.offset(name)

    def _aview(self, arena, name):
        return self.layout.view(arena, name)

    def _bn_views(self, arena, bs: BNSpec, n=4):
        """The first n of a BN's arena tensors: weight, bias, running_mean, running_var."""
        return [self._aview(arena, f"{bs.name}.{k}") for k in _BN_PARAMS[:n]]

    def _red(self, bs: BNSpec, which: str):
        bp = self.plan.bns[bs.name]
        off, rows = (bp.fwd_off, 2) if which == "fwd" else (bp.bwd_off, 3)
        return self.red[off:off + self.plan.slot_words * rows * bs.c]

    def _ctr(self, bs: BNSpec, which: int) -> int:
        return self.red.data_ptr() + 4 * (self.plan.bns[bs.name].ctr + which)

    def _fin_fwd(self, bs: BNSpec, arena, count):
        """The in-launch forward finalize descriptor of bs (cached per arena and count)."""
        key = ("f", bs.name, arena.data_ptr(), count)
        if key not in self._fins:
            st = self.bn[bs.name]
            self._fins[key] = K.bn_fin(*self._bn_views(arena, bs), st["affine"], st["saved"], self._ctr(bs, 0), count,
                                       self.eps, self.mom, bs.c, sshift=st["sshift"], sshift_next=st["sshift_next"])
        return self._fins[key]

    def _fin_bwd(self, bs: BNSpec, arena, count):
        key = ("b", bs.name, arena.data_ptr(), count)
        if key not in self._fins:
            st = self.bn[bs.name]
            self._fins[key] = K.bn_bwd_fin(self._aview(arena, f"{bs.name}.weight"), st["saved"], st["coef"],
                                           self._gptr(f"{bs.name}.weight"), self._gptr(f"{bs.name}.bias"),
                                           self._ctr(bs, 1), count, 1.0, bs.c, self.grad_fp16)
        return self._fins[key]

    def _conv_bn_fwd(self, cs: ConvSpec, x, y, bs: BNSpec, arena, train: bool, bn_in=None):
        """conv -> (train) batch statistics + BN finalize | (eval) running-statistics affine.
        With conv v2 the finalize can run inside the conv launch (last workgroup, bnfin.hpp)."""
        p, fin_at = self.plan.convs[cs.name], self.plan.bns[bs.name].fwd_fin
        oh, ow = cs.out_hw
        npix = self.B * oh * ow
        stats = self._red(bs, "fwd") if train else None
        sshift = self.bn[bs.name]["sshift"] if train else None
        assert bn_in is None or p.wino, cs.name
        if p.wino:
            uf, _, v = self.wu[cs.name]
            self._wino_late_wait(p)
            if p.fwd == "wino_fused":
                K.wino_fused(x, uf, y, None, stats, v, self.B, cs.h, cs.w, cs.cp, cs.cout, bn_in=bn_in, sshift=sshift)
            else:
                K.wino_conv(x, uf, y, None, stats, v if v is not None else self.wino_s2, self.wino_s1, self.B, cs.h,
                            cs.w, cs.cp, cs.cout, bn_in=bn_in, sshift=sshift)
        else:
            wf = self.wbuf[p.wf_off:p.wf_off + cs.cout * cs.kg]
            if p.fwd == "stem":
                if not K.stem_conv(x, wf, y, stats, self.B, cs.h, cs.w, cs.cin, cs.cp, cs.cout, cs.kg, sshift=sshift,
                                   k=cs.k):
                    raise RuntimeError(f"{cs.name}: the planned direct stem kernel refused the shape")
            else:
                fin = self._fin_fwd(bs, arena, npix) if (train and fin_at == "conv") else None
                K.conv_fwd2(x, wf, y, stats, self.wpart, self.B, cs.h, cs.w, cs.cp, cs.cout, cs.k, cs.stride, cs.pad,
                            cs.kg, fin=fin, sshift=sshift)
        if not train:
            self._bn_eval(bs, arena)
        elif fin_at == "separate":
            self._bn_train(bs, arena, self.nslots, npix)

    def _apply(self, bs: BNSpec, y, out, arena, train: bool, res=None, bs2: BNSpec | None = None):
        """BN (+ residual, + shortcut BN bs2 on res) + ReLU; with bn_finalize "apply" the
        training-mode finalize of bs (and bs2) runs inside this launch."""
        c = bs.c
        if train and self.plan.bns[bs.name].fwd_fin == "apply":
            npix = y.numel() // c
            two = dict(part2=self._red(bs2, "fwd"), fin2=self._fin_fwd(bs2, arena, npix)) if bs2 is not None else {}
            K.bn_apply_fin(y, self._red(bs, "fwd"), self._fin_fwd(bs, arena, npix), out, c, relu=True, res=res, **two)
            return
        K.bn_apply(y, self.bn[bs.name]["affine"], out, c, relu=True, res=res,
                   affine2=self.bn[bs2.name]["affine"] if bs2 is not None else None)

    def _bn_train(self, bs: BNSpec, arena, T, count):
        st = self.bn[bs.name]
        w, b, rm, rv = self._bn_views(arena, bs)
        K.bn_finalize(self._red(bs, "fwd"), T, bs.c, count, w, b, self.eps, self.mom, rm, rv, st["affine"],
                      st["saved"], sshift=st["sshift"], sshift_next=st["sshift_next"])

    def _bn_eval(self, bs: BNSpec, arena):
        K.bn_eval_affine(bs.c, *self._bn_views(arena, bs), self.eps, self.bn[bs.name]["affine"])

    def _side(self):
        """Weight gradients only feed the push, so they run on a side stream concurrently with
        the dgrad -> BN-backward critical path (ordered after their dy by an event; joined at
        the end of every backward segment)."""
        if self.wg_stream is None:
            return contextlib.nullcontext()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.wg_stream.wait_event(ev)
        return torch.cuda.stream(self.wg_stream)

    def join_side(self):
        if self.wg_stream is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.wg_stream)

    def _wgrad(self, cs: ConvSpec, x, dy, fold=None):
        if self._wg_batch is not None:  # deferred: issued together at the end of the unit
            self._wg_batch.append((cs, x, dy, fold))
            return
        with self._side():
            self._wgrad_now(cs, x, dy, fold)

    def _flush_wgrads(self):
        batch, self._wg_batch = self._wg_batch, None
        if batch:
            with self._side():
                for cs, x, dy, fold in batch:
                    self._wgrad_now(cs, x, dy, fold)

    def _wgrad_now(self, cs: ConvSpec, x, dy, fold=None, scratch=None):
        """cs's weight gradient by its planned route. fold: the BN-backward apply in front of it is
        folded into its dy load (_grad_operands); scratch = (dy tiles, partials) of the tail one."""
        p = self.plan.convs[cs.name]
        wd, wpart = scratch if scratch is not None else (self.wino_wd, self.wino_wpart) if p.wino else (None, None)
        if p.wgrad == "wgrad2":
            assert fold is None, cs.name
            part = self.wpart_w[p.wp_off:p.wp_off + p.wp]
            K.conv_wgrad2(x, dy, part, self.B, cs.h, cs.w, cs.cp, cs.cout, cs.k, cs.stride, cs.pad, cs.kg)
            item = (part, p.splits, cs.cout, cs.kg, cs.cin, cs.cp, cs.k, self._gptr(f"{cs.name}.weight"))
            if p.rbatch:
                self._wr_batch.append(item)  # reduced with the block's other layers (_flush_reduces)
            else:
                K.wgrad_reduce(*item[:7], 1.0, item[7], self.grad_fp16)
            return
        out = self.layout.grad_view(self.grads, f"{cs.name}.weight")  # straight into the wire: nothing to reduce
        if p.wgrad == "wino_fused":
            xf = self.xsrc.get(cs.name)  # its input was never written: y + the BN affine instead
            K.wino_wgrad_fused(xf[0] if xf else x, dy, wpart, out, self.B, cs.h, cs.w, cs.cp, cs.cout,
                               xaff=xf[1] if xf else None, bwd_in=fold)
        elif p.wgrad == "wino_dz":
            # both operands from one pass over dy (with ``fold``: over dz, the BN apply folded in
            # and its coefficients published): D here, V' left in wino_s1 for _dgrad, which
            # follows; nothing of the weight-gradient chain touches wino_s1
            # rounded as the apply pass (as_apply): the step equals the unfolded one bit for bit
            K.check(K.wino_dz_xf(dy, self.wino_s1, wd, self.B, cs.h, cs.w, cs.cout, bwd_in=fold, as_apply=True),
                    "wino_dz_xf")
            K.wino_wgrad_pre(self.wu[cs.name][2], wd, wpart, out, self.B, cs.h, cs.w, cs.cp, cs.cout)
        else:
            K.wino_wgrad(self.wu[cs.name][2], dy, wd, wpart, out, self.B, cs.h, cs.w, cs.cp, cs.cout, bwd_in=fold)

    def _flush_reduces(self):
        batch, self._wr_batch = self._wr_batch, None
        if batch:
            with self._side():
                K.wgrad_reduce_batch(batch, 1.0, self.grad_fp16)

    def _dgrad(self, cs: ConvSpec, dy, dx, res=None, bn_next=None, sc=None, fold=None):
        """cs's data gradient by its planned route. bn_next = (BNSpec, o, y, two|None): the BN whose
        backward consumes dx; where the plan says so its reduction (sum dz, sum dz*xhat) is
        produced by this launch's epilogue. sc = (shortcut ConvSpec, its output gradient) on the
        "conv2_sc" route: the block's 1x1 / stride-2 shortcut data gradient folded into this
        3x3 / stride-2 launch. fold: as for _wgrad_now."""
        p = self.plan.convs[cs.name]
        bst = None
        if bn_next is not None and self.plan.bns[bn_next[0].name].bwd_sums == "dgrad":
            bs, o, y, two = bn_next
            st, ms = self.bn[bs.name], self.plan.bns[bs.name].premasked
            if bs.name in self.plan.bnfold:  # o was never written: the mask comes from the affine
                bst = K.bwd_stats_desc(self._red(bs, "bwd"), None, y, st["saved"], mask_store=ms,
                                       mask_aff=st["affine"])
            else:
                y2, saved2 = (two[1], self.bn[two[0].name]["saved"]) if two is not None else (None, None)
                bst = K.bwd_stats_desc(self._red(bs, "bwd"), o, y, st["saved"], y2, saved2, mask_store=ms)
        geo = (self.B, cs.h, cs.w, cs.cout, cs.cp)
        if p.wino:  # Winograd: the output transform produces the same fused sums
            ud = self.wu[cs.name][1]
            if p.dgrad == "wino_fused":
                K.wino_fused(dy, ud, dx, res, None, None, *geo, bst=bst, bwd_in=fold)
            elif p.dgrad == "wino_pre":  # its transformed input is in wino_s1 already (_wgrad_now)
                K.wino_conv_pre(self.wino_s1, ud, dx, res, None, self.wino_s2, *geo, bst=bst)
            else:
                assert fold is None, cs.name  # a folded dy exists in no buffer
                K.wino_conv(dy, ud, dx, res, None, self.wino_s1, self.wino_s2, *geo, bst=bst)
            return
        wd = self.wbuf[p.wd_off:p.wd_off + cs.cp * cs.kgd]
        if p.dgrad == "conv2_sc":
            ds, dys_sc = sc
            pd = self.plan.convs[ds.name]
            if not K.conv_dgrad2_sc(dy, wd, dx, self.wpart, self.B, cs.h, cs.w, cs.cp, cs.cout, cs.kgd, dys_sc,
                                    self.wbuf[pd.wd_off:pd.wd_off + ds.cp * ds.kgd], ds.kgd, bst=bst):
                raise RuntimeError(f"{cs.name}: the planned shortcut fold was refused")
            return
        K.conv_dgrad2(dy, wd, dx, res, self.wpart, self.B, cs.h, cs.w, cs.cp, cs.cout, cs.k, cs.stride, cs.pad,
                      cs.kgd, bst=bst)

    def _bn_bwd(self, bs: BNSpec, arena, g, o, y, dx, npix, two=None, dzout=None):
        """BN (+ReLU mask from o) backward; two = (bs2, y2, dx2) for a shared-dz second BN.
        Returns the buffer that holds dz = g*[o > 0]: ``g`` itself when the producing dgrad stored
        it masked, else ``dzout`` (written here when given)."""
        bp, st, part = self.plan.bns[bs.name], self.bn[bs.name], self._red(bs, "bwd")
        if bp.premasked:
            o = dzout = None
        pre = bp.bwd_sums != "reduce"  # sums already produced by a dgrad epilogue or the head
        bs2, y2, dx2 = two if two is not None else (None, None, None)
        st2 = self.bn[bs2.name] if bs2 is not None else None

        def fin(b, on=True):
            return self._fin_bwd(b, arena, npix) if on and b is not None else None

        if self.opts.bn_finalize == "apply":  # finalize inside the apply launch
            if not pre:
                K.bn_bwd_reduce(g, o, y, st["saved"], part, npix, bs.c, y2=y2, saved2=st2 and st2["saved"])
            K.bn_bwd_apply_fin(g, o, y, part, fin(bs), dx, bs.c, y2=y2, fin2=fin(bs2), dx2=dx2, dzout=dzout)
            return g if bp.premasked else dzout
        fuse = self.opts.bn_finalize == "conv" and not pre  # finalize in the reduce launch's last block
        T = self.nslots if pre else K.bn_bwd_reduce(g, o, y, st["saved"], part, npix, bs.c, y2=y2,
                                                    saved2=st2 and st2["saved"], fin1=fin(bs, fuse),
                                                    fin2=fin(bs2, fuse))
        if not fuse:
            for which, (b_, s_) in enumerate([(bs, st)] + ([(bs2, st2)] if bs2 is not None else []), 1):
                K.bn_bwd_finalize(part, T, 2 if bs2 is None else 3, which, b_.c, npix,
                                  self._aview(arena, f"{b_.name}.weight"), s_["saved"], s_["coef"],
                                  self._gptr(f"{b_.name}.weight"), self._gptr(f"{b_.name}.bias"), 1.0, self.grad_fp16)
        K.bn_bwd_apply(g, o, y, st["coef"], dx, bs.c, y2=y2, coef2=st2 and st2["coef"], dx2=dx2, dzout=dzout)
        return g if bp.premasked else dzout


    # ------------------------------------------------------------------ public API
    def unpack(self, arena: torch.Tensor):
        """OIHW master weights -> bf16 implicit-GEMM operands. The source is the fp32 arena, or
        the bf16 weight image ``self.wsrc`` when the fetch delivers one (parallel/codec.py
        WeightWire: the server's apply wrote those bits; identical operands either way)."""
        src = self.wsrc if self.wsrc is not None else arena
        K.param_unpack_tiles(src, self.descs, self.ndesc, self.ntiles, self.wbuf, scatter=self.small_scatter)
        if self.wu:
            self._wino_unpack(arena)

    def set_weight_source(self, img: torch.Tensor | None, pre_unpack=None, scatter=None):
        """Read conv weights from a bf16 image (same offsets as the arena's parameter prefix)
        instead of the fp32 arena. The fp32 remainder reaches the local arena either through
        ``scatter`` = (src, idx, dst, gather), done by extra workgroups of the unpack launch
        (kernels.param_unpack_tiles), or through ``pre_unpack``, run first inside every captured
        step. Invalidates graphs."""
        if img is not None:
            assert not self.f32, "the fp32 engine unpacks its operands from the fp32 arena (fetch codec fp32)"
            assert img.dtype == torch.bfloat16 and img.numel() >= self.layout.param_numel
        assert scatter is None or (img is not None and pre_unpack is None)
        self.wsrc = img
        self.pre_unpack = pre_unpack
        self.small_scatter = scatter
        self.graph = None
        self.graphs = None

    def load_batch(self, images_u8, labels_all, train=True):
        """Gather self.index rows of the HBM-resident dataset + fused crop/flip/normalize."""
        H, W = self.spec.in_hw
        # a training step's per-step zeroing (BN statistic slots, accuracy counter) rides on the
        # augment launch (forward/head then skip their own zero_ launches)
        zero = (self.red, self.correct) if train else None
        self._zeroed_head = train
        K.augment(images_u8, labels_all, self.index, self.x0, self.labels, self.B, H, W, 4, self.seed, self.step_dev,
                  train, self.mean, self.std, zero=zero,
                  copy=(self.bn_shift[1], self.bn_shift[0]) if train else None)
        self._zeroed = train

    def forward(self, arena: torch.Tensor, train: bool = True):
        # the kernel library's deterministic-reduction state is process-wide host state: every
        # step (and every captured graph) takes this engine's setting
        K.set_deterministic(self.deterministic)
        sp, B = self.spec, self.B
        st = sp.stem_conv
        zeroed, self._zeroed = self._zeroed, False
        if train and not zeroed:
            self.red.zero_()
            self.bn_shift[0].copy_(self.bn_shift[1])  # this step's statistic shifts (see _build)
        self._conv_bn_fwd(st, self.x0, self.y0, sp.stem_bn, arena, train)
        self._apply(sp.stem_bn, self.y0, self.a0, arena, train)
        if sp.maxpool:
            K.maxpool3s2_fwd(self.a0, self.p0, self.pidx)
        for b, d in zip(sp.blocks, self.blk):
            src = d["inp"]
            L = len(b.convs)
            bn_in = None
            for i, cs in enumerate(b.convs):
                self._conv_bn_fwd(cs, src, d["y"][i], b.bns[i], arena, train, bn_in=bn_in)
                bn_in = None
                if i < L - 1:
                    bs = b.bns[i]
                    if train and self.plan.bns[bs.name].fwd_fin == "next_conv":  # applied by its input transform
                        bn_in = (self._red(bs, "fwd"), self._fin_fwd(bs, arena, d["y"][i].numel() // bs.c))
                        src = d["y"][i]
                        continue
                    self._apply(bs, d["y"][i], d["a"][i], arena, train)
                    src = d["a"][i]
            if b.down:
                ds, dbn = b.down
                self._conv_bn_fwd(ds, d["inp"], d["ys"], dbn, arena, train)
                self._apply(b.bns[-1], d["y"][-1], d["out"], arena, train, res=d["ys"], bs2=dbn)
            else:
                self._apply(b.bns[-1], d["y"][-1], d["out"], arena, train, res=d["inp"])
        return self.final

    def head(self, arena: torch.Tensor, backward: bool = True):
        sp = self.spec
        zeroed, self._zeroed_head = self._zeroed_head, False
        if not zeroed:
            self.correct.zero_()
        # the last block's output BN: its backward sums come out of the head launch (one
        # bn_bwd_reduce pass fewer) when the fused per-sample head runs and that BN has no
        # shortcut BN sharing its gradient
        bst = None
        if backward and sp.blocks and self.plan.bns[sp.blocks[-1].bns[-1].name].bwd_sums == "head":
            last = sp.blocks[-1].bns[-1]
            bst = K.bwd_stats_desc(self._red(last, "bwd"), self.final, self.blk[-1]["y"][-1],
                                   self.bn[last.name]["saved"])
        fused = K.head_fwd_bwd(self.final, self.B, self.head_hw, sp.fc_in, self._aview(arena, f"{sp.fc}.weight"),
                               self._aview(arena, f"{sp.fc}.bias"), sp.classes, self.labels, self.pooled,
                               self.dlogits, self.dfinal if backward else None, self.loss, self.correct, bst=bst)
        if bst is not None and not fused:
            raise RuntimeError("the head did not produce the planned BN-backward sums")

    def _bwd_fc(self, arena):
        sp = self.spec
        with self._side():
            K.head_wgrad(self.dlogits, self.pooled, self.B, sp.classes, sp.fc_in, self._gptr(f"{sp.fc}.weight"),
                         self._gptr(f"{sp.fc}.bias"), 1.0, self.grad_fp16)

    def _bwd_block(self, arena, j: int):
        """Backward of residual block j; its incoming gradient is the next block's input grad.
        With the side stream its weight gradients are issued as one batch after the block, and its
        direct ones' split-K partials reduced by one launch (plan: ConvPlan.rbatch)."""
        self._wg_batch = [] if self.wg_stream is not None else None
        self._wr_batch = []
        try:
            self._bwd_block_body(arena, j)
        finally:
            self._flush_wgrads()
            self._flush_reduces()

    def _split_tail(self) -> bool:
        """The tail weight gradient (ConvPlan.tail) leaves block 0's batch for the compute stream,
        after the stem's BN backward (_bwd_stem), concurrently with the side stream's instead of
        after it: only when block 0 and the stem end in the same backward segment (a gradient
        bucket is pushed when its segment ends)."""
        if not self.plan.tail_split:
            return False
        if self.segments is None:
            return True
        key = ".".join(self.spec.blocks[0].convs[0].name.split(".")[:2])
        return any(key in g and "stem" in g for g in self.segments)

    def _gin(self, j: int, i: int):
        """The gradient wrt the output of block j's BN i (+ ReLU)."""
        d = self.blk[j]
        if i < len(d["da"]):
            return d["da"][i]
        return self.blk[j + 1]["gin"] if j + 1 < len(self.blk) else self.dfinal

    def _grad_operands(self, arena, j: int, i: int):
        """(x, dy, fold) that the gradients of block j's conv i read. Where the BN-backward apply in
        front of it is folded (PSX_TUNE wino_bwdfold=1, default: the conv has the fused Winograd
        data gradient and a Winograd weight gradient, the BN's incoming gradient is already the
        masked dz and its sums came from the producing dgrad's epilogue) there is no apply pass:
        dy = k1 dz + k2 y + k3 is formed inside both consumers' operand loads (wino_fused.hip,
        wino.hip dy transform) from fold = (y, sums, finalize descriptor), and the fused data
        gradient publishes the coefficients and dgamma / dbeta. A three-launch "wino_dz" layer
        folds too: its one pass over dz (wino.hip wino_dz_xf_kernel) is both consumers' load and the
        publisher, and rounds dy as the apply pass would (bit-equal to the unfolded step)."""
        b, d = self.spec.blocks[j], self.blk[j]
        x = d["inp"] if i == 0 else d["a"][i - 1]
        if not self.plan.convs[b.convs[i].name].bwd_fold:
            return x, d["dy"][i], None
        g, bs = self._gin(j, i), b.bns[i]
        return x, g, (d["y"][i], self._red(bs, "bwd"), self._fin_bwd(bs, arena, g.numel() // bs.c))

    def _bn_bwd_to(self, arena, j: int, i: int, dzout=None):
        """The backward of block j's BN i, whose output gradient feeds only conv i's gradients: a
        pass of its own unless folded into them (_grad_operands). Returns the buffer holding dz."""
        b, d = self.spec.blocks[j], self.blk[j]
        g, bs = self._gin(j, i), b.bns[i]
        if self.plan.bns[bs.name].bwd_apply == "folded":
            return g
        o = d["a"][i] if i < len(d["a"]) else d["out"]
        return self._bn_bwd(bs, arena, g, o, d["y"][i], d["dy"][i], g.numel() // bs.c, dzout=dzout)

    def _bwd_block_body(self, arena, j: int):
        b, d = self.spec.blocks[j], self.blk[j]
        L = len(b.convs)
        if b.down:
            ds, dbn = b.down
            g = self._gin(j, L - 1)
            self._bn_bwd(b.bns[-1], arena, g, d["out"], d["y"][-1], d["dy"][-1], g.numel() // dbn.c,
                         two=(dbn, d["ys"], d["dys"]))
        else:
            dz = self._bn_bwd_to(arena, j, L - 1, dzout=d["dz"])
        for i in range(L - 1, -1, -1):
            cs = b.convs[i]
            x, dy, fold = self._grad_operands(arena, j, i)
            if not (self.plan.convs[cs.name].tail and self._split_tail()):
                self._wgrad(cs, x, dy, fold)
            if i > 0:
                self._dgrad(cs, dy, d["da"][i - 1], bn_next=(b.bns[i - 1], d["a"][i - 1], d["y"][i - 1], None),
                            fold=fold)
                self._bn_bwd_to(arena, j, i - 1)
            elif b.down:
                self._wgrad(ds, d["inp"], d["dys"])
                # the 1x1 / stride-2 shortcut's data gradient folded into the 3x3 / stride-2 one
                # (a layer the kernel cannot fold: two launches + a residual pass)
                if self.plan.convs[cs.name].dgrad == "conv2_sc":
                    self._dgrad(cs, dy, d["gin"], bn_next=self._bn_into(j), sc=(ds, d["dys"]))
                else:
                    self._dgrad(ds, d["dys"], d["dxs"])
                    self._dgrad(cs, dy, d["gin"], res=d["dxs"], bn_next=self._bn_into(j), fold=fold)
            else:
                self._dgrad(cs, dy, d["gin"], res=dz, bn_next=self._bn_into(j), fold=fold)

    def _bn_into(self, j: int):
        """The BN whose backward consumes block j's input gradient: the previous block's output
        BN (+ its shortcut BN), or the stem BN (not across the ResNet-50 max-pool)."""
        if j > 0:
            pb, pd = self.spec.blocks[j - 1], self.blk[j - 1]
            two = (pb.down[1], pd["ys"]) if pb.down else None
            return (pb.bns[-1], pd["out"], pd["y"][-1], two)
        if self.spec.maxpool:
            return None
        return (self.spec.stem_bn, self.a0, self.y0, None)

    def _bwd_stem(self, arena):
        sp, B = self.spec, self.B
        st = sp.stem_conv
        p, q = st.out_hw
        g = self.blk[0]["gin"] if self.blk else self.dfinal
        if sp.maxpool:
            K.maxpool3s2_bwd(g, self.pidx, self.g0)
            g = self.g0
        self._bn_bwd(sp.stem_bn, arena, g, self.a0, self.y0, self.dy0, B * p * q)
        self._wgrad(st, self.x0, self.dy0)
        if self._split_tail():  # the step's tail weight gradient, beside the side stream's
            self._wgrad_now(sp.blocks[0].convs[0], *self._grad_operands(arena, 0, 0), scratch=self.wino_tail)

    def backward_units(self, arena):
        """The backward pass as (unit key, thunk) in execution order. Unit keys name the
        gradient-arena region each unit finalizes: "fc", "layer<i>.<j>" (one residual block),
        "stem" (conv1 + bn1) — the same keys as parallel/overlap.py:unit_key, so a gradient
        bucket can be pushed as soon as the units that write it have run."""
        units = [("fc", lambda: self._bwd_fc(arena))]
        for j in range(len(self.spec.blocks) - 1, -1, -1):
            key = ".".join(self.spec.blocks[j].convs[0].name.split(".")[:2])
            units.append((key, lambda j=j: self._bwd_block(arena, j)))
        units.append(("stem", lambda: self._bwd_stem(arena)))
        return units

    def backward(self, arena: torch.Tensor):
        for _, fn in self.backward_units(arena):
            fn()
        self.join_side()

    def set_segments(self, groups):
        """Split the backward into segments (lists of unit keys, in backward order) so that a
        callback can run — and a bucket's collective be issued — between them."""
        keys = [k for k, _ in self.backward_units(None)]
        flat = [k for grp in groups for k in grp]
        if flat != keys:
            raise ValueError(f"segments {groups} do not cover the backward units {keys}")
        self.segments = [list(g) for g in groups]
        self.graph = None
        self.graphs = None

    def _segment_fns(self, arena, images_u8, labels_all, unpack):
        units = dict(self.backward_units(arena))
        groups = self.segments or [[k for k, _ in self.backward_units(arena)]]

        def prologue():
            if unpack:
                if self.pre_unpack is not None:
                    self.pre_unpack()
                self.unpack(arena)
            if images_u8 is not None:
                self.load_batch(images_u8, labels_all, train=True)
            self.forward(arena, train=True)
            self.head(arena, backward=True)

        fns = []
        for si, grp in enumerate(groups):
            def seg(grp=grp, first=(si == 0)):
                if first:
                    prologue()
                for k in grp:
                    units[k]()
                self.join_side()  # a segment's gradients are complete when it ends
            fns.append(seg)
        return fns

    def train_step(self, arena: torch.Tensor, images_u8=None, labels_all=None, unpack=True, on_segment=None):
        """unpack (optional) + batch load + forward + loss + backward -> self.grads.
        ``on_segment(i)`` runs after backward segment i has been issued (see set_segments)."""
        for si, fn in enumerate(self._segment_fns(arena, images_u8, labels_all, unpack)):
            fn()
            if on_segment is not None:
                on_segment(si)

    def reset_stat_shift(self):
        """Forget the BN statistic shifts (the previous batch means, see _build): the next step
        sums plainly, as the first step of a fresh engine does."""
        self.bn_shift.zero_()

    # ------------------------------------------------------------------ graphs
    def capture(self, arena, images_u8, labels_all, unpack=True, warmup=2):
        """Capture the step into HIP graphs (one per backward segment, all sharing one memory
        pool); replay with ``step_graph()``."""
        shift = self.bn_shift.clone()  # the warm-up steps' batch means must not become the first replay's shifts
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self.train_step(arena, images_u8, labels_all, unpack)
        torch.cuda.current_stream().wait_stream(s)
        self.bn_shift.copy_(shift)
        graphs = []
        for fn in self._segment_fns(arena, images_u8, labels_all, unpack):
            g = torch.cuda.CUDAGraph()
            # thread-local capture: in torch's default (global) mode any other thread's stream
            # synchronize, allocation or copy invalidates the capture (hipErrorStreamCaptureInvalidated,
            # profiles/r6_capture_probe.jsonl) — the co-located async server's comm thread does all
            # three while this worker thread captures its first step (docs/ARCHITECTURE.md)
            with torch.cuda.graph(g, pool=graphs[0].pool() if graphs else None, capture_error_mode="thread_local"):
                fn()
            graphs.append(g)
        self.graphs = graphs
        self.graph = graphs[0]
        return graphs[0]

    def step_graph(self, on_segment=None):
        for si, g in enumerate(self.graphs):
            g.replay()
            if on_segment is not None:
                on_segment(si)

    def evaluate_batch(self, arena, images_u8, labels_all):
        self.load_batch(images_u8, labels_all, train=False)
        self.forward(arena, train=False)
        self.head(arena, backward=False)
