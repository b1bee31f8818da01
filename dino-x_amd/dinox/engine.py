"""Training engine: one DINO-X optimiser step on the HIP kernels, optionally data-parallel.

Follows the order of the reference loop (scripts/phase5_big_run.py:1692-1802) for
``--loss-type dino`` with ``accumulation_steps == 1``:

    lr = get_lr(step)                                              :1692-1700
    student fwd, teacher fwd (no grad), heads on CLS                :1741-1747
    DINO loss with the PRE-update centre, then centre EMA           :1749-1755 -> :692-720
    + gram_weight * Gram anchoring loss                             :1758-1761
    + koleo_weight * KoLeo regulariser on the student head output   :1764-1766
    backward                                                        :1772
    global grad-norm, AdamW (wd on every parameter), EMA teacher    :1781-1802

``loss_type="simclr"`` (:1728-1737): student fwd, student head on CLS, NT-Xent loss on the two halves of the logits
(ops.ntxent_fwd / ntxent_bwd), backward, grad-norm + AdamW.  No teacher forward, no Gram, no KoLeo, no centre update and -- as
the reference applies it for ``dino`` only (:1799) -- no EMA: teacher arena and centre stay bit-identical.  Single rank, no
multi-crop (cross-rank negatives are not implemented).

``loss_type="mae"`` (:1627-1632, :1724-1727): the student is a ``dinox.mae.MaeModel`` and there is no teacher: forward with random
masking, reconstruction loss on the removed patches (ops.mae_loss_fwd / mae_loss_bwd), backward, AdamW.  No head, centre or EMA.
The parameters the MAE graph never reaches (``encoder.registers``, ``encoder.scale_embed.*``, the fixed ``decoder.decoder_pos_embed``)
form the TAIL of the arena and the optimiser pass runs over the prefix only, so they stay bit-identical (the reference's AdamW skips
``.grad is None``).  The logged grad-norm is the reference's: over the ENCODER's gradients (its loop walks ``student.parameters()``,
and the MAE decoder is not part of ``student``, :1785).  Single rank, eager launches, fp32 image batches only.

``ibot_weight > 0`` (extension, dino only; iBOT / DINOv2): ``step(..., patch_mask=)`` names the patches of the global views that the student
sees as ``backbone.mask_token``; their final-norm tokens, student and teacher, go through the same heads as the CLS rows (appended to the
same operands) and ``ops.ibot_ce`` scores them against a patch centre of their own (``ibot_center``).  With the weight 0 -- or nothing
masked on a step -- the step is launch for launch the one above.

What is different from the reference, by design:
  * parameters, gradients, Adam moments and teacher weights live in flat fp32 arenas, so the grad-norm,
    AdamW and EMA are ONE kernel pass (dinox_adamw_ema) instead of 161 x (.item() + 2 EMA launches); the dW products
    accumulate straight into the gradient arena (ops._GradSink), which is zeroed once per optimiser step;
  * no host synchronisation inside a step: loss and grad-norm stay on the device until asked for;
  * data parallel: bucketed RCCL all-reduce of the gradient arena overlapped with backward, centre
    batch-mean all-reduced, 1/world folded into the AdamW kernel (dinox/dp.py).
Documented deviation: the reference's AdamW skips parameters whose ``.grad`` is None (only possible for
``scale_embed.*`` when a scale-aware model is stepped with ``spacing=None``); the arena pass applies
weight decay to them.  The reference loop always passes spacing for scale-aware models (:1713).
"""
from __future__ import annotations

import gc
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist

from . import ops
from .dp import GradBucketer, exchanging
from .schedule import get_lr


@dataclass
class StepHyperParams:
    """Defaults are the reference CLI defaults (scripts/phase5_big_run.py:1264-1285)."""
    lr: float = 1e-4
    min_lr: float = 1e-6
    warmup_steps: int = 2500
    max_steps: Optional[int] = None
    weight_decay: float = 0.04
    ema: float = 0.996
    teacher_temp: float = 0.04
    student_temp: float = 0.1
    center_momentum: float = 0.9
    gram_weight: float = 1.0
    koleo_weight: float = 0.0
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    loss_type: str = "dino"          # "dino" | "simclr" (SimCLRLoss on the student head output, reference :1728-1737) | "mae"
    simclr_temp: float = 0.1         # the reference hard-codes SimCLRLoss(temperature=0.1)
    mae_mask_ratio: float = 0.75     # the reference hard-codes MaeModel(mask_ratio=0.75); the engine sets it on the model it is given
    centering: str = "ema"           # "ema" (the reference's centre) | "sinkhorn" (DINOv2/v3 Sinkhorn-Knopp targets; extension, dino only)
    sk_iters: int = 3                # Sinkhorn-Knopp iterations (DINOv2: 3)
    simclr_negatives: str = "local"  # "local" (one rank's batch; single rank only) | "global" (the rows of every rank: extension, simclr only)
    ibot_weight: float = 0.0         # weight of the iBOT masked-patch term (extension, dino only; 0: the step is exactly the one without it)


def flatten_parameters(module: torch.nn.Module, align: int = 8, order: Optional[List[torch.nn.Parameter]] = None
                       ) -> Tuple[torch.Tensor, List[torch.nn.Parameter], List[int]]:
    """Move every parameter of ``module`` into one flat fp32 arena (each at an offset of a multiple of 8 elements, so that
    both the fp32 slice and the same slice of a bf16 image of the arena are 16-byte aligned) and re-point ``p.data`` at its slice.  Returns (arena, params in arena order, element offsets).
    ``order``: the same parameters in another arena order (default: ``module.parameters()``)."""
    params = list(module.parameters())
    if order is not None:
        if len(order) != len(params) or {id(p) for p in order} != {id(p) for p in params}:
            raise ValueError("order must be a permutation of module.parameters()")
        params = list(order)
    if not params:
        raise ValueError("module has no parameters")
    dev = params[0].device
    offsets, total = [], 0
    for p in params:
        if p.dtype != torch.float32:
            raise TypeError("master parameters must be fp32")
        offsets.append(total)
        total += (p.numel() + align - 1) // align * align
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    for p, off in zip(params, offsets):
        flat[off:off + p.numel()].copy_(p.data.reshape(-1))
        p.data = flat[off:off + p.numel()].view(p.shape)
    return flat, params, offsets


class TrainEngine:
    """Owns student/teacher arenas, the DINO centre and the optimiser state; ``step()`` runs one update."""

    def __init__(self, student: torch.nn.Module, teacher: torch.nn.Module, out_dim: int, hp: StepHyperParams,
                 amp_dtype: Optional[torch.dtype] = None, process_group=None, bucket_bytes: int = 32 << 20,
                 accumulation_steps: int = 1, use_graph: bool = False) -> None:
        """``use_graph``: after two eager steps the whole optimiser step (forward, backward, optimiser tail) is captured ONCE into
        a hipGraph and every later step is one graph launch -- for the launch-bound small-batch regime (at bs 64 the host needs
        10-14 ms to enqueue the ~700 launches of a step that the GPU finishes in 11).  The C ABI was designed for it: no
        allocation, no synchronisation, no host-dependent scalar inside a launch (lr and the Adam bias corrections come from
        device memory, dinox_adamw_ema_dev).  Single rank, accumulation_steps == 1, fixed batch shape.

        The objective is chosen here, once: ``self._objective`` runs forward, loss and backward between ``_begin`` and ``_finish``,
        and what it lacks it declares -- ``bucketer`` None (no gradient exchange), no teacher in ``spans`` (no EMA stage), no batch
        mean returned (no centre move)."""
        self.student, self.teacher, self.hp = student, teacher, hp
        if accumulation_steps < 1:
            raise ValueError("accumulation_steps must be >= 1")
        self.accum = accumulation_steps
        self.compute_dtype = amp_dtype or torch.float32
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        if hp.loss_type not in ("dino", "simclr", "mae"):
            raise ValueError(f"loss_type must be 'dino', 'simclr' or 'mae', got {hp.loss_type!r}")
        if hp.centering not in ("ema", "sinkhorn"):
            raise ValueError(f"centering must be 'ema' or 'sinkhorn', got {hp.centering!r}")
        if hp.sk_iters < 1:
            raise ValueError(f"sk_iters must be >= 1, got {hp.sk_iters}")
        if hp.centering == "sinkhorn" and hp.loss_type != "dino":
            raise ValueError(f"centering='sinkhorn' shapes the teacher targets of loss_type='dino'; loss_type={hp.loss_type!r} has none")
        if hp.simclr_negatives not in ("local", "global"):
            raise ValueError(f"simclr_negatives must be 'local' or 'global', got {hp.simclr_negatives!r}")
        if hp.simclr_negatives == "global" and hp.loss_type != "simclr":
            raise ValueError(f"simclr_negatives='global' belongs to loss_type='simclr'; loss_type={hp.loss_type!r} has no negatives")
        if hp.ibot_weight < 0.0:
            raise ValueError(f"ibot_weight must be >= 0, got {hp.ibot_weight}")
        self.ibot = hp.ibot_weight > 0.0
        if self.ibot and hp.loss_type != "dino":
            raise ValueError(f"ibot_weight > 0 adds the masked-patch term to loss_type='dino' (it shares the DINO head and teacher); "
                             f"loss_type={hp.loss_type!r} has neither")
        if self.ibot and use_graph:
            raise ValueError("ibot_weight > 0 does not run under use_graph: the number of masked patches changes from step to step and a "
                             "captured step has one fixed layout")
        if hp.loss_type == "mae":
            self._mae_arena(student, teacher, use_graph)
        else:
            self._two_net_arenas(student, teacher, process_group, bucket_bytes)
        dev = self.flat_p.device
        self.center = torch.zeros(1, out_dim, dtype=torch.float32, device=dev)      # (mae never reads it; a checkpoint's "dino_loss" entry holds it)
        if self.ibot:
            if not self.manual_top:
                raise ValueError("ibot_weight > 0 needs the stock DINO head (Linear -> GELU -> Linear with biases): the masked rows join the "
                                 "CLS rows in the hand-written top of the step, which a replaced head does not take")
            if any(getattr(m.backbone, "mask_token", None) is None for m in (student, teacher)):
                raise ValueError("ibot_weight > 0 needs backbones built with mask_token=True (student and teacher share one arena layout)")
            self.ibot_center = torch.zeros(1, out_dim, dtype=torch.float32, device=dev)     # the patch centre: apart from the CLS centre
        self._ibot_pending = None        # (column sums + count of this step's masked teacher rows, their all-reduce): awaited in _finish
        self.use_graph = bool(use_graph)
        if self.use_graph and (self.accum != 1 or exchanging(process_group)):
            raise ValueError("use_graph: single rank and accumulation_steps == 1 only")
        self._hyper_dev = torch.zeros(3, dtype=torch.float32, device=dev)
        self._hyper_host = torch.zeros(3, dtype=torch.float32).pin_memory() if dev.type == "cuda" else torch.zeros(3)
        self._graph = None
        self._static: Optional[list] = None
        self._eager_steps = 0
        self._zero1 = torch.zeros(1, dtype=torch.float32, device=dev)
        self.marks = None            # bench.py: a list -> (phase name, HIP event on the launch stream) at every phase boundary of step()
        self.step_count = 0          # micro-batches seen (drives the LR schedule, like the reference)
        self.opt_steps = 0           # optimiser steps taken (AdamW bias correction)
        self.last = {}

    def _build_arena(self, module: torch.nn.Module, order=None, n_optimised: Optional[int] = None) -> None:
        """flat_p / params / offsets of ``module`` (flatten_parameters) with gradient and Adam-moment arenas of the same layout;
        ``p.grad`` of the first ``n_optimised`` parameters (default: all) is its slice of the gradient arena."""
        self.flat_p, self.params, self.offsets = flatten_parameters(module, order=order)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.adam_m = torch.zeros_like(self.flat_p)
        self.adam_v = torch.zeros_like(self.flat_p)
        self.sunk = self.params[:n_optimised]             # what the gradient sink knows: the rest keeps .grad = None
        for p, off in zip(self.sunk, self.offsets):
            p.grad = self.flat_g[off:off + p.numel()].view(p.shape)

    def _two_net_arenas(self, student, teacher, process_group, bucket_bytes) -> None:
        """dino and simclr: a student and a teacher arena of one layout, gradient buckets, the teacher's side stream."""
        simclr = self.hp.loss_type == "simclr"
        if simclr and self.world > 1 and self.hp.simclr_negatives != "global":
            raise ValueError("loss_type='simclr' runs on a single rank only (the negatives of a row are the rows of ONE batch; "
                             "cross-rank negatives are not implemented) unless simclr_negatives='global' gathers them from every rank")
        # simclr_negatives="global": NT-Xent over the rows of every rank (ops.ntxent_fwd(group=)); None keeps the square single-rank kernels
        # (ops takes group=None as "no exchange", so the default process group is named)
        self._ntxent_group = None
        if simclr and self.hp.simclr_negatives == "global" and dist.is_initialized():
            self._ntxent_group = process_group if process_group is not None else dist.group.WORLD
        for p in teacher.parameters():
            p.requires_grad_(False)
        self._build_arena(student)
        self.flat_t, t_params, t_off = flatten_parameters(teacher)
        if t_off != self.offsets or self.flat_t.numel() != self.flat_p.numel():
            raise ValueError("student and teacher must have identical parameter layouts")
        if exchanging(process_group):                        # identical start on every rank
            dist.broadcast(self.flat_p, src=0, group=process_group)
            dist.broadcast(self.flat_t, src=0, group=process_group)
        dev = self.flat_p.device
        self.bucketer = GradBucketer(self.params, self.offsets, self.flat_g, bucket_bytes=bucket_bytes, group=process_group)
        self.bucketer.pre_exchange = ops.dw_stream.join
        # the teacher forward has no data dependence on the student forward: it runs on its own HIP stream so the two
        # kernel chains fill each other's tails (every launch ends with a partial last round of workgroups)
        self.side_stream = torch.cuda.Stream(device=dev) if dev.type == "cuda" else None
        self.shadows = [ops.ArenaShadow(self.flat_p, self.params, self.offsets), ops.ArenaShadow(self.flat_t, t_params, t_off)]
        # simclr: no teacher pointer -> the optimiser pass has no EMA stage and the teacher arena is not touched (ema = 1.0 would still
        # rewrite every element as 1.0 * t + 0.0 * w, which turns -0.0 into +0.0 and is NaN where w is not finite)
        self.spans = [(0, self.flat_p.numel(), None if simclr else self.flat_t)]
        import zoo.arch as _arch
        self.manual_top = all(type(m.head) is _arch.DinoHead and type(m.head[0]) is _arch.Linear and type(m.head[2]) is _arch.Linear
                              and m.head[0].bias is not None and m.head[2].bias is not None for m in (student, teacher)) \
            and not os.environ.get("DINOX_AUTOGRAD_TOP")
        self._objective = self._simclr_objective if simclr else self._dino_objective
        self._no_local_crops = "loss_type='simclr' takes the two global views only (no local crops)" if simclr else None

    def _mae_arena(self, student, teacher, use_graph) -> None:
        """One arena [encoder, reached | decoder, reached | never reached], no teacher arena; the optimiser sees the first two parts."""
        from .mae import MaeModel
        if not isinstance(student, MaeModel):
            raise ValueError(f"loss_type='mae' takes a dinox.mae.MaeModel as the student (encoder + decoder), got {type(student).__name__}")
        if teacher is not None:
            raise ValueError("loss_type='mae' has no teacher: pass teacher=None")
        if self.world > 1:
            raise ValueError("loss_type='mae' runs on a single rank only (data-parallel MAE is not implemented)")
        if use_graph:
            raise ValueError("loss_type='mae' does not support use_graph (the step is launched eagerly)")
        student.mask_ratio = self.hp.mae_mask_ratio
        enc, dec = student.encoder, student.decoder
        tail_ids = {id(dec.decoder_pos_embed)}
        if getattr(enc, "num_registers", 0) > 0:
            tail_ids.add(id(enc.registers))
        if getattr(enc, "scale_aware", False):
            tail_ids.update(id(p) for p in enc.scale_embed.parameters())
        enc_ids = {id(p) for p in enc.parameters()}
        every = list(student.parameters())
        head = [p for p in every if id(p) in enc_ids and id(p) not in tail_ids]
        body = [p for p in every if id(p) not in enc_ids and id(p) not in tail_ids]
        tail = [p for p in every if id(p) in tail_ids]
        pos_of = {id(p): i for i, p in enumerate(every)}
        self._build_arena(student, order=head + body + tail, n_optimised=len(head) + len(body))
        self.state_index = [pos_of[id(p)] for p in self.params]      # position in student.parameters(): the optimiser-state keys of a checkpoint
        ends = self.offsets + [self.flat_p.numel()]
        enc_end, opt_end = ends[len(head)], ends[len(head) + len(body)]      # (multiples of 8: slices stay 16-byte aligned)
        # two optimiser passes; the logged grad-norm is the first one's, over the ENCODER's gradients, as the reference's is
        self.spans = [(0, enc_end, None), (enc_end, opt_end, None)]
        self.flat_t = self.bucketer = self.side_stream = None
        self.shadows = [ops.ArenaShadow(self.flat_p, self.params, self.offsets)]
        self.manual_top = False
        self._objective = self._mae_objective
        self._no_local_crops = "loss_type='mae' takes the global views only (no local crops)"

    def _mark(self, name: str) -> None:
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    # -- one optimiser step ---------------------------------------------------------------------
    def step(self, batch: torch.Tensor, spacing2b: Optional[torch.Tensor] = None, local_batch: Optional[torch.Tensor] = None,
             local_spacing: Optional[torch.Tensor] = None, mask_noise: Optional[torch.Tensor] = None, patch_mask=None) -> dict:
        """batch: (2B,3,H,W) = [view1; view2] on the device; spacing2b: (2B,3) or None.
        local_batch (L*B,3,s,s), view-major, with local_spacing (L*B,3): the multi-crop extension (not in the reference, dino only) --
        the student also sees L smaller crops per sample, which enter the DINO term only (every (teacher view, other student
        view) pair, averaged); Gram and KoLeo stay on the global views.
        ``loss_type="mae"``: batch (V,3,H,W) fp32 -- every view is one sample, as in the reference (:1725); spacing is ignored there and
        here.  ``mask_noise`` ([V, L] fp32, mae only): the noise whose per-sample order decides which patches are kept; None draws it
        from torch's global device generator.
        ``patch_mask`` (``ibot_weight > 0`` only): (idx, w, tok) of ``dinox.ibot`` on the device, or a ``dinox.ibot.PatchMask`` -- the masked
        patches of the global views (flat positions v * P + i, int32, distinct and ascending), their loss weights 1 / n_v (fp32) and their
        rows v * N + 1 + i of the token matrix (int32).  None or empty: nothing is masked on this step and the term is 0.
        Returns device tensors {loss, dino, gram, koleo, grad_norm_sq} (plus simclr / mae with that ``loss_type``) and the python
        float lr (no sync)."""
        mae = self.hp.loss_type == "mae"          # (refusals come before anything is launched or counted)
        if mask_noise is not None and not mae:
            raise ValueError("mask_noise belongs to loss_type='mae'")
        if local_batch is not None and self._no_local_crops:
            raise ValueError(self._no_local_crops)
        if mae and isinstance(batch, ops.PatchOperand):
            raise ValueError("loss_type='mae' takes the fp32 image batch (the loss reads its pixels), not a PatchOperand")
        if patch_mask is not None and not self.ibot:
            raise ValueError("patch_mask belongs to ibot_weight > 0")
        if patch_mask is not None:
            idx, w, tok = patch_mask.triple() if hasattr(patch_mask, "triple") else patch_mask
            if len(idx) == 0:
                patch_mask = None
            else:
                if not (len(idx) == len(w) == len(tok)) or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (idx, w, tok)):
                    raise ValueError("patch_mask must be (idx, w, tok): three device tensors of one length (dinox.ibot.PatchMask.to(device))")
                patch_mask = (idx, w, tok)
        if not self.use_graph:
            return self._step_eager(batch, spacing2b, local_batch, local_spacing, mask_noise, patch_mask=patch_mask)
        return self._step_graph([batch, spacing2b, local_batch, local_spacing])

    def _step_graph(self, inputs: list) -> dict:
        hp = self.hp
        if self._graph is None and self._eager_steps < 2:       # eager first: LDS limits granted, operand images and tables built
            self._eager_steps += 1
            return self._step_eager(*inputs)
        lr = get_lr(self.step_count, hp.max_steps, hp.warmup_steps, hp.lr, hp.min_lr)
        # a FRESH page-locked staging tensor per step (the host allocator recycles it only after the copy has run): with one reused
        # buffer a host running two steps ahead would overwrite the scalars of a copy that is still queued
        self._hyper_host = torch.tensor(ops.adamw_hyper(lr, hp.beta1, hp.beta2, self.opt_steps + 1), dtype=torch.float32).pin_memory()
        self._hyper_dev.copy_(self._hyper_host, non_blocking=True)
        if self._graph is None:
            self._static = [None if t is None else t.clone() for t in inputs]
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            count, opt = self.step_count, self.opt_steps
            # No cyclic garbage collection while the stream captures.  An engine is a reference cycle (self._objective is a bound
            # method), so a dead one -- with its CUDAGraph, its graph-pool tensors and its page-locked staging buffer -- waits for
            # the collector, and a collection that fires inside the capture destroys them through API calls that a capturing
            # thread may not make: the process aborts.  torch.cuda.graph() no longer collects on entry, so collect here.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(self._graph):
                    self._captured = self._step_eager(*self._static, hyper=self._hyper_dev)
            finally:
                if gc_was_on:
                    gc.enable()
            self.step_count, self.opt_steps = count, opt          # capturing enqueued nothing: the replay below IS this step
        else:
            for dst, src in zip(self._static, inputs):
                if (dst is None) != (src is None) or (dst is not None and dst.shape != src.shape):
                    raise ValueError("use_graph: the batch layout must not change after capture")
                if dst is not None:
                    dst.copy_(src, non_blocking=True)
        self._graph.replay()
        self.step_count += 1
        self.opt_steps += 1
        self.last = dict(self._captured, lr=lr)
        return self.last

    def _step_eager(self, batch, spacing2b=None, local_batch=None, local_spacing=None, mask_noise=None, hyper: Optional[torch.Tensor] = None,
                    patch_mask=None) -> dict:
        """The skeleton every objective shares.  The objective returns (its scalars by name, batch mean of the teacher output or None, the
        batch mean's pending all-reduce or None)."""
        self._patch_mask = patch_mask
        lr, last = self._begin()
        scalars, bm, bm_work = self._objective(batch, spacing2b, local_batch, local_spacing, mask_noise)
        return self._finish(lr, last, hyper, scalars, bm, bm_work)

    def _begin(self):
        hp = self.hp
        lr = get_lr(self.step_count, hp.max_steps, hp.warmup_steps, hp.lr, hp.min_lr)
        # gradient accumulation with the reference's semantics (phase5_big_run.py:1769-1796): `step` counts micro-batches,
        # loss/accum is back-propagated every micro-batch, the optimiser (and EMA) run when (step+1) % accum == 0 with the LR
        # of that micro-batch, the centre moves every micro-batch.  Gradients are exchanged once, on the last micro-batch.
        first = self.step_count % self.accum == 0
        last = (self.step_count + 1) % self.accum == 0
        self._mark("start")
        if first:
            ops.zero_(self.flat_g)
        on_ready = None
        if self.bucketer is not None:
            self.bucketer.active = last
            self.bucketer.arm()
            if self.bucketer.exchange:
                on_ready = self.bucketer.grad_ready
        if ops.grad_sink.owner is not self:      # weight gradients accumulate straight into flat_g (ops._GradSink)
            ops.grad_sink.register(self, self.sunk, on_ready)
            ops.weight_cache.shadows = self.shadows
        ops.grad_sink.uses.clear()
        return lr, last

    def _finish(self, lr, last, hyper, scalars, bm, bm_work) -> dict:
        """Everything after the backward pass: centre EMA, gradient exchange, grad-norm + AdamW (+ teacher EMA) over ``spans``."""
        hp = self.hp
        ops.dw_stream.join()              # (weight-gradient products enqueued on the dW stream, when DINOX_DW_STREAM is set)
        self._mark("bwd")
        if bm_work is not None:
            bm_work.wait()
            bm.div_(self.world)           # (data parallel only)
        if bm is not None:
            ops.center_ema_(self.center.view(-1), bm, hp.center_momentum)
        if self._ibot_pending is not None:         # the patch centre moves like the CLS centre (untouched when no row was masked anywhere)
            sum_count, work = self._ibot_pending
            self._ibot_pending = None
            if work is not None:
                work.wait()
            ops.ibot_center_ema_(self.ibot_center.view(-1), sum_count, hp.center_momentum)
        if self.bucketer is not None:
            self.bucketer.finish()
        self._mark("comm_exposed")        # what of the exchanges did not fit under backward (+ the centre EMA launch)
        if last:
            self.opt_steps += 1
            norms = [ops.adamw_ema_(self.flat_p[lo:hi], self.flat_g[lo:hi], self.adam_m[lo:hi], self.adam_v[lo:hi],
                                    None if teacher is None else teacher[lo:hi], lr=lr, weight_decay=hp.weight_decay, beta1=hp.beta1,
                                    beta2=hp.beta2, eps=hp.adam_eps, step_t=self.opt_steps, ema=hp.ema, grad_scale=1.0 / self.world, hyper=hyper)
                     for lo, hi, teacher in self.spans]
            gsq = norms[0]
            ops.weight_cache.clear()     # master weights changed under the bf16 copies
            if self.compute_dtype == torch.bfloat16:
                for sh in self.shadows:  # one cast launch per arena (+ one for every transposed matrix backward uses)
                    sh.refresh()
        else:
            gsq = self._zero1                                # the reference logs grad-norm 0 between optimiser steps
        self._mark("optimiser_tail")
        self.step_count += 1
        z = self._zero1
        named = {k: (z if v is None else v).detach().reshape(()) for k, v in scalars.items()}
        # (dino / gram / koleo: every objective reports them, as zeros where it has none -- callers rely on the keys)
        self.last = {"loss": named.pop("loss"), "dino": named.pop("dino", z.reshape(())), "gram": named.pop("gram", z.reshape(())),
                     "koleo": named.pop("koleo", z.reshape(())), "grad_norm_sq": gsq, "lr": lr, **named}
        return self.last

    # -- the objectives: forward, loss, backward -----------------------------------------------------------------------
    def _dino_objective(self, batch, spacing2b, local_batch, local_spacing, mask_noise):
        # (the unfolded batch is shared by student and teacher WITHIN this scope, never carried across steps)
        with ops.compute_dtype(self.compute_dtype), ops.unfold_share():
            main = torch.cuda.current_stream()
            # opt-in (DINOX_SIDE_STREAM=1): +1.3 % measured, but concurrent chains blur per-kernel timings, so bench/profiles keep it off
            side = self.side_stream if os.environ.get("DINOX_SIDE_STREAM") else None
            if side is not None:
                ops.patch_unfold(batch, self.student.backbone.patch, self.compute_dtype)     # shared by both nets: before the fork
                side.wait_stream(main)
                with torch.cuda.stream(side), torch.no_grad():
                    t_feats = self.teacher.backbone(batch, spacing=spacing2b)
                s_feats = self._student_forward(batch, spacing2b)
                main.wait_stream(side)
                t_feats.record_stream(main)
            else:
                s_feats = self._student_forward(batch, spacing2b)
                self._mark("fwd_student")
                with torch.no_grad():
                    t_feats = self.teacher.backbone(batch, spacing=spacing2b)
                self._mark("fwd_teacher")
            if self.manual_top:
                return self._losses_and_backward(s_feats, t_feats, local_batch, local_spacing)
            with torch.no_grad():
                t_out = self.teacher.head(t_feats[:, 0])
            return self._losses_and_backward_autograd(s_feats, t_feats, t_out, batch, local_batch, local_spacing)

    def _student_forward(self, batch, spacing2b):
        """The student's global views; with a patch mask on this step the masked patches enter as ``backbone.mask_token``."""
        if self._patch_mask is None:
            return self.student.backbone(batch, spacing=spacing2b)
        return self.student.backbone(batch, spacing=spacing2b, patch_idx=self._patch_mask[0])

    def _mae_objective(self, batch, spacing2b, local_batch, local_spacing, mask_noise):
        """Forward with random masking, reconstruction loss on the removed patches, backward (no unfold sharing: one net, one forward)."""
        model = self.student
        with ops.compute_dtype(self.compute_dtype):
            pred_full, ids_restore = model.forward_full(batch, mask_noise)
            self._mark("fwd_student")
            with torch.no_grad():
                loss, saved = ops.mae_loss_fwd(pred_full.detach(), batch, ids_restore, model.len_keep, model.encoder.patch, lead=1)
                dpred = ops.mae_loss_bwd(saved, 1.0 / self.accum)
            self._mark("loss")
            torch.autograd.backward([pred_full], [dpred])
        return {"loss": loss, "mae": loss}, None, None

    def _target_center(self, t_out: torch.Tensor) -> torch.Tensor:
        """The centre the cross-entropy subtracts from the teacher logits.  "ema": the running centre, as in the reference.  "sinkhorn":
        the vector c of THIS batch's teacher rows for which softmax((t - c) / teacher_temp) are the Sinkhorn-Knopp targets (ops.sk_center;
        all global views in one problem, over the global batch under data parallelism).  The EMA centre is maintained either way."""
        if self.hp.centering == "sinkhorn":
            return ops.sk_center(t_out, self.hp.teacher_temp, self.hp.sk_iters, group=self.group)
        return self.center

    # -- everything above the backbones, without the framework's elementwise kernels ---------------------------------
    def _head(self, head, cls_op: torch.Tensor, train: bool):
        """DinoHead = Linear(D,D) -> GELU -> Linear(D,out) (zoo/arch.py:252-256) on the CLS rows, by the MLP core of ops: (logits fp32, saved)."""
        l0, l2 = head[0], head[2]
        return ops.mlp_forward(cls_op, l0.weight, l0.bias, l2.weight, l2.bias, None, torch.float32, self.compute_dtype, train)

    def _student_head_backward(self, saved, ds: torch.Tensor) -> torch.Tensor:
        """d logits [V,out] fp32 -> d CLS rows [V,D]; the four parameter gradients go straight into the gradient arena."""
        dt = self.compute_dtype
        l0, l2 = self.student.head[0], self.student.head[2]
        dcls, *sunk = ops.mlp_backward(saved, ops.to_mode(ds, dt), l0.weight, l0.bias, l2.weight, l2.bias, dt, True)
        assert sunk == [None] * 4, "the head's parameters must live in the engine's gradient arena"
        return dcls

    def _losses_and_backward(self, s_feats, t_feats, local_batch, local_spacing):
        """Heads, DINO CE (pre-update centre), Gram, KoLeo and the gradient of their weighted sum w.r.t. the student features, written
        out by hand -- every step is one of the library's kernels -- then ONE autograd backward from the features down.  (Through
        autograd the same thing costs a strided CLS copy + cast per head, `ds * g` / `d * g` multiplies, a zero fill + slice copy +
        158 MB add to merge the two feature gradients, and a handful of scalar kernels: ~0.35 ms of framework kernels per step.)"""
        hp, dt = self.hp, self.compute_dtype
        scale = 1.0 / self.accum
        V = s_feats.shape[0]
        # iBOT: the M masked patch rows of student and teacher ride at the END of the heads' operands -- one head product each way for CLS,
        # local-crop and patch rows -- and the cross-entropies see their own rows of the logits.  M = 0 (or the term off): the step below is
        # launch for launch the one without it.
        mask = self._patch_mask
        M = 0 if mask is None else mask[0].numel()
        with torch.no_grad():
            sf = s_feats.detach()
            t_op = ops.take_rows(t_feats, 0, dt, out_rows=V + M)
            if M:
                ops.gather_rows(t_feats, mask[2], dt, out=t_op, out_row0=V)
            t_all, _ = self._head(self.teacher.head, t_op, train=False)
            t_out = t_all[:V] if M else t_all
            if local_batch is None:
                l_feats, n_loc = None, 0
                cls = ops.take_rows(sf, 0, dt, out_rows=V + M)
            else:
                with torch.enable_grad():
                    l_feats = self.student.backbone(local_batch, spacing=local_spacing)
                lf = l_feats.detach()
                n_loc = lf.shape[0]
                cls = ops.take_rows(sf, 0, dt, out_rows=V + n_loc + M)
                ops.take_rows(lf, 0, dt, out=cls, out_row0=V)
            if M:
                ops.gather_rows(sf, mask[2], dt, out=cls, out_row0=V + n_loc)
            s_all, saved = self._head(self.student.head, cls, train=True)
            center = self._target_center(t_out)
            ds_all = torch.empty_like(s_all) if M else None
            s_dino, ds_dino = (s_all[:V + n_loc], ds_all[:V + n_loc]) if M else (s_all, None)
            if local_batch is None:
                l_dino, ds = ops.dino_ce(s_dino, t_out, center, hp.student_temp, hp.teacher_temp, True, grad_scale=scale, ds_out=ds_dino)
            else:
                l_dino, ds = ops.dino_ce_multi(s_dino, t_out, center, hp.student_temp, hp.teacher_temp, 2, grad_scale=scale, ds_out=ds_dino)
            l_ibot = None
            if self.ibot:
                l_ibot = self._ibot_term(s_all, t_all, ds_all, V, n_loc, M, scale)
            # centre EMA after the loss used the old centre; batch mean is global under DP (the centre itself moves after backward,
            # so the exchange runs under the backward pass)
            bm = ops.colmean(t_out)
            bm_work = dist.all_reduce(bm, op=dist.ReduceOp.SUM, group=self.group, async_op=True) if exchanging(self.group) else None
            # KoLeo (:1764-1766; nearest neighbours over the global batch under DP): its all-gather of the unit rows is started here and
            # awaited after the Gram loss, which has no data in common with it (nor with the head's backward)
            kstate = ops.koleo_begin(s_all[:V], group=self.group) if hp.koleo_weight > 0.0 else None
            dfeats = torch.empty_like(sf)
            l_gram = None
            if hp.gram_weight != 0.0:
                l_gram, gsaved = ops.gram_loss_fwd(sf, t_feats, dt)
                ops.gram_loss_bwd(gsaved, tuple(sf.shape), hp.gram_weight * scale, dfeats=dfeats, accumulate=False)   # rows 1..N-1
            else:
                ops.zero_(dfeats)
            l_koleo = None
            if kstate is not None:
                l_koleo, ksaved = ops.koleo_end(kstate)
                ops.axpy_(ds[:V], ops.koleo_bwd(ksaved, hp.koleo_weight * scale), 1.0)      # (ds[:V]: the leading rows, contiguous)
            dcls = self._student_head_backward(saved, ds_all if M else ds)
            ops.put_rows_(dfeats, 0, dcls)                                                                            # row 0 (CLS)
            if M:                                                             # the masked patch rows, on top of what Gram wrote there
                ops.scatter_add_rows_(dfeats, mask[2], dcls, src_row0=V + n_loc)
            roots, grads = [s_feats], [dfeats]
            if l_feats is not None:
                dl = torch.empty_like(lf)
                ops.zero_(dl)
                ops.put_rows_(dl, 0, dcls, src_row0=V)
                roots.append(l_feats)
                grads.append(dl)
            loss = ops.lincomb3(l_dino, l_gram, l_koleo, hp.gram_weight, hp.koleo_weight)
            if l_ibot is not None:
                loss = ops.lincomb3(loss, l_ibot, None, hp.ibot_weight, 0.0)
        self._mark("loss")
        torch.autograd.backward(roots, grads)
        scalars = {"loss": loss, "dino": l_dino, "gram": l_gram, "koleo": l_koleo}
        if self.ibot:
            scalars["ibot"] = l_ibot                      # (None on a step without masked rows: reported as 0)
        return scalars, bm, bm_work

    def _ibot_term(self, s_all, t_all, ds_all, V: int, n_loc: int, M: int, scale: float):
        """The masked-patch cross-entropy on the trailing M rows of the heads' outputs (its gradient into the same rows of ``ds_all``) and the
        patch centre's bookkeeping: (column sums, count) of the masked teacher rows, all-reduced under data parallelism -- every rank
        takes part on every step, M differs per rank and may be 0 -- and handed to ``_finish``.  Returns the loss [1], or None at M = 0."""
        hp = self.hp
        dp = exchanging(self.group)
        K = t_all.shape[1]
        sum_count = None
        l_ibot = None
        if M:
            idx, w_rows, tok = self._patch_mask
            s_p, t_p = s_all[V + n_loc:], t_all[V:]
            if hp.centering == "sinkhorn":
                c_p = ops.sk_center(t_p, hp.teacher_temp, hp.sk_iters, group=self.group)
            else:
                c_p = self.ibot_center
            l_ibot, _, _ = ops.ibot_ce(s_p, t_p, c_p, w_rows, hp.student_temp, hp.teacher_temp, scale=1.0 / V, grad_scale=hp.ibot_weight * scale,
                                       ds_out=ds_all[V + n_loc:])
            sum_count = torch.empty(K + 1, dtype=torch.float32, device=t_all.device)
            ops.colsum(t_p, out=sum_count[:K])
            count = torch.tensor([float(M)], dtype=torch.float32)          # (a fresh page-locked word per step, like the AdamW scalars)
            sum_count[K:].copy_(count.pin_memory() if t_all.is_cuda else count, non_blocking=True)
        elif dp:
            if hp.centering == "sinkhorn":
                ops.sk_center_idle(K, hp.sk_iters, self.group, t_all.device)
            sum_count = torch.empty(K + 1, dtype=torch.float32, device=t_all.device)
            ops.zero_(sum_count)
        if sum_count is not None:
            work = dist.all_reduce(sum_count, op=dist.ReduceOp.SUM, group=self.group, async_op=True) if dp else None
            self._ibot_pending = (sum_count, work)
        return l_ibot

    def _simclr_objective(self, batch, spacing2b, local_batch, local_spacing, mask_noise):
        """Student forward, student head on the CLS rows, NT-Xent on the two halves of its output (reference :1729-1737) and the backward
        pass.  With the stock head: by hand, like _losses_and_backward -- head products, ops.ntxent_fwd / ntxent_bwd, head backward, the
        CLS gradient into a zeroed feature gradient, ONE autograd backward from the features down.  Otherwise through the per-op
        autograd nodes."""
        hp, dt = self.hp, self.compute_dtype
        with ops.compute_dtype(dt), ops.unfold_share():
            s_feats = self.student.backbone(batch, spacing=spacing2b)
            self._mark("fwd_student")
            if not self.manual_top:
                s_out = self.student.head(s_feats[:, 0])
                half = s_out.shape[0] // 2
                loss = ops.simclr_loss(s_out[:half], s_out[half:], hp.simclr_temp, group=self._ntxent_group)
                self._mark("loss")
                (loss if self.accum == 1 else loss / self.accum).backward()
            else:
                with torch.no_grad():
                    sf = s_feats.detach()
                    z, saved = self._head(self.student.head, ops.take_rows(sf, 0, dt), train=True)
                    loss, nsaved = ops.ntxent_fwd(z, hp.simclr_temp, group=self._ntxent_group)
                    dcls = self._student_head_backward(saved, ops.ntxent_bwd(nsaved, 1.0 / self.accum))
                    dfeats = torch.empty_like(sf)
                    ops.zero_(dfeats)
                    ops.put_rows_(dfeats, 0, dcls)                                                                        # row 0 (CLS)
                self._mark("loss")
                torch.autograd.backward([s_feats], [dfeats])
        return {"loss": loss, "simclr": loss}, None, None

    def _losses_and_backward_autograd(self, s_feats, t_feats, t_out, batch, local_batch, local_spacing):
        """The same through the per-op autograd nodes (a head whose layers were replaced, e.g. LoRA-wrapped)."""
        hp = self.hp
        with torch.no_grad():
            center = self._target_center(t_out)
        if local_batch is None:
            s_out = self.student.head(s_feats[:, 0])
            l_dino = ops.DinoCEFn.apply(s_out, t_out, center, hp.student_temp, hp.teacher_temp)
        else:
            l_feats = self.student.backbone(local_batch, spacing=local_spacing)
            s_all = self.student.head(torch.cat([s_feats[:, 0], l_feats[:, 0]], 0))       # one head product for all views
            s_out = s_all[:s_feats.shape[0]]
            l_dino = ops.DinoCEMultiFn.apply(s_all, t_out, center, hp.student_temp, hp.teacher_temp, 2)
        bm = ops.colmean(t_out)
        bm_work = dist.all_reduce(bm, op=dist.ReduceOp.SUM, group=self.group, async_op=True) if exchanging(self.group) else None
        if hp.gram_weight != 0.0:
            l_gram = ops.GramLossFn.apply(s_feats, t_feats)
            loss = l_dino + hp.gram_weight * l_gram
        else:
            l_gram = torch.zeros((), device=batch.device)
            loss = l_dino
        if hp.koleo_weight > 0.0:
            l_koleo = ops.koleo_loss(s_out, group=self.group)
            loss = loss + hp.koleo_weight * l_koleo
        else:
            l_koleo = torch.zeros((), device=batch.device)
        self._mark("loss")            # (local-crop forward, student head, DINO CE, Gram, KoLeo forward)
        (loss if self.accum == 1 else loss / self.accum).backward()
        return {"loss": loss, "dino": l_dino, "gram": l_gram, "koleo": l_koleo}, bm, bm_work

    # -- convenience ------------------------------------------------------------------------------
    def scalars(self) -> dict:
        """Host copies of the last step's scalars (this is the only place that synchronises): what the objective returned (simclr adds
        the key "simclr", mae "mae", ibot_weight > 0 "ibot"; a dino engine without it returns exactly the keys it always did, so whatever
        iterates over them sees no new entry), the grad-norm and the lr."""
        out = {}
        for k, v in self.last.items():
            if k == "grad_norm_sq":
                out["grad_norm"] = float(v) ** 0.5
            else:
                out[k] = v if k == "lr" else float(v)
        return out
