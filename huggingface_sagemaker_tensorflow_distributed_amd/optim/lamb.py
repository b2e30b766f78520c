"""Fused LAMB over the flat parameter store (``--optimizer lamb``): layer-wise trust ratios for large batches.

The math is TF Addons' ``tfa.optimizers.LAMB`` (You et al., "Large Batch Optimization for Deep Learning"). With ``g``
the gradient averaged over ranks and accumulation micro-steps (``grad_scale · grad``, times the clip coefficient when
``max_grad_norm`` is on) and ``t`` the 1-based step::

    m = β1 m + (1-β1) g          v = β2 v + (1-β2) g²
    m̂ = m / (1-β1ᵗ)              v̂ = v / (1-β2ᵗ)
    u = m̂ / (√v̂ + ε)  [+ wd · w   for segments with decay]
    r = ‖w‖₂ / ‖u‖₂  if ‖w‖₂ > 0 and ‖u‖₂ > 0 else 1     (per segment, over the fp32 master weight)
    w ← w − lr · r · u

* Layer adaptation is excluded for the segments weight decay is excluded for (biases and LayerNorm parameters,
  ``Segment.decay == False``): TF Addons' ``exclude_from_layer_adaptation`` falls back to
  ``exclude_from_weight_decay``, and it is the usual BERT recipe. Those segments take ``r = 1`` and no decay.
* A NaN norm compares false and gives ``r = 1``. There is no trust-ratio clamp (TF Addons has none).
* Defaults: β = (0.9, 0.999), ε = 1e-6 (TF Addons), ``weight_decay`` as given. There is no ``eps_mode``: LAMB always
  uses the bias-corrected form above.
* Tied weights are one parameter, so one segment. The alignment padding between segments is zero in ``master``,
  ``grad``, ``m`` and ``v``; it yields ``u = 0`` and contributes to no norm.
* Per-parameter learning rates (``lr_multipliers``, as :class:`FusedAdam`'s): ``w ← w − ((lr·μ)·r)·u`` with ``μ``
  the segment's fp32 multiplier. ``u``, the norms and ``r`` do not depend on ``μ``: the ``(r, Σw², Σu²)`` table a step
  writes is the same bits with and without multipliers. The kernel reads ``μ`` from an fp32 ``[segments]`` table.
* Weight averaging (``ema_decay``, as :class:`FusedAdam`'s): the weight-update kernel also writes
  ``ema ← ema + ω·(w_new − ema)``; ``u``, the norms, ``r`` and every other output do not see it. Captured steps read
  ``ω`` from :attr:`dcoef` slot 6.
* The Horovod-style scripts keep multiplying the learning rate by the world size (``train/runner.py``); LAMB does not
  change that rule.

GPU path (``csrc/kernels/lamb.hip``): per slice of whole segments, three launches -- moments and per-tile
``(Σw², Σu²)`` partials, one workgroup per segment for ``r``, then the weight update with the bf16 copy (or the fp32
run's hi / lo halves) in the same pass. No atomics and a fixed combine order: two runs, and a slice-by-slice run
against a whole-buffer one, give the same bits. The norms are per segment, so -- unlike global-norm clipping -- the
slices stay overlapped with the backward (:meth:`FusedAdam.enable_overlap`). Nothing returns to the host: every launch
captures into the whole-step HIP graph, where the per-step scalars come from :attr:`dcoef`, fp32 ``[8]`` =
``(lr, 1/(1-β1ᵗ), 1/(1-β2ᵗ), ε, grad_scale, wd, 1 - ema decay, -)``.

With ``max_grad_norm > 0`` the clip structure of :class:`FusedAdam` is kept: the hooks run ``grad_sumsq`` per slice
under the backward, and :meth:`step` finishes the norm and runs LAMB over the whole buffer with the device-side
coefficient (LAMB with a global clip of 1.0 is the standard BERT recipe).

CPU path (``master`` not on a GPU): the same math with torch ops per segment, norms in fp64.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from ..parallel.flat_params import ALIGN, FlatParamStore
from .adam import FusedAdam


class FusedLamb(FusedAdam):
    kind = "lamb"

    def __init__(self, store: FlatParamStore, lr: float = 1e-3, betas=(0.9, 0.999), eps: Optional[float] = None,
                 weight_decay: float = 0.0, max_grad_norm: float = 0.0, lr_multipliers=None,
                 ema_decay: float = 0.0, ema_warmup: bool = False):
        super().__init__(store, lr=lr, betas=betas, eps=1e-6 if eps is None else eps, weight_decay=weight_decay,
                         eps_mode="keras", max_grad_norm=max_grad_norm, lr_multipliers=lr_multipliers,
                         ema_decay=ema_decay, ema_warmup=ema_warmup)
        segs = store.segments
        dev = store.master.device
        self._spans = [(segs[i + 1].offset if i + 1 < len(segs) else (s.offset + s.numel + ALIGN - 1) // ALIGN * ALIGN)
                       - s.offset for i, s in enumerate(segs)]
        # (r, Σw², Σu²) of the last step per segment; on the GPU the kernels write it (no host round trip)
        self._ratio = torch.zeros(len(segs), 3, dtype=torch.float32, device=dev)
        self._ratio[:, 0] = 1.0
        self._plan = None
        self._partials: Optional[torch.Tensor] = None
        self._seg_ranges: List[Tuple[int, int]] = []
        self._dclip: Optional[torch.Tensor] = None
        if store.master.is_cuda:
            from ..ops import hip

            # tile / segment tables and workspaces on the device, at addresses that stay put (captured graphs)
            self._plan = hip.lamb_plan([s.offset for s in segs], self._spans, [s.decay for s in segs], store.numel,
                                       store.master)
            self._partials = torch.zeros(2 * self._plan.ntiles, dtype=torch.float32, device=dev)

    def _build_lr_table(self) -> None:
        """LAMB's table: one fp32 entry per segment (the weight-update kernel knows each tile's segment)."""
        self._lr_mul = self._mu.to(self.store.master.device)

    # -------------------------------------------------------------------------- trust ratios
    @property
    def last_trust_ratios(self) -> torch.Tensor:
        """Device tensor ``[segments]``: the last step's ``r`` per segment (1 on excluded segments)."""
        return self._ratio[:, 0]

    def trust_ratios(self) -> Dict[str, float]:
        """``{segment name: r}`` of the last step. Synchronises with the device: call it only when logging."""
        return dict(zip(self.store.names, self._ratio[:, 0].tolist()))

    def trust_ratio_summary(self) -> Tuple[float, float, float]:
        """(min, median, max) of the last step's ratios over the adapted segments (a device read: logging only)."""
        r = [x for x, s in zip(self._ratio[:, 0].tolist(), self.store.segments) if s.decay] or [1.0]
        r.sort()
        return r[0], r[len(r) // 2], r[-1]

    # -------------------------------------------------------------------------- state
    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["kind"] = self.kind
        return sd

    def _coeffs(self):
        """LAMB's per-step scalars: the two bias corrections ``1 / (1-β1ᵗ)``, ``1 / (1-β2ᵗ)`` (where Adam keeps its
        bias-corrected step and effective ε: :meth:`begin_step` stores whichever pair with the gradient scale)."""
        t = self.step_count
        return 1.0 / (1.0 - self.beta1 ** t), 1.0 / (1.0 - self.beta2 ** t)

    # -------------------------------------------------------------------------- device-side coefficients
    def use_device_coef(self) -> torch.Tensor:
        """The fp32 [8] device tensor ``(lr, 1/(1-β1ᵗ), 1/(1-β2ᵗ), ε, grad_scale, wd, 1 - ema decay, -)`` that LAMB
        launches captured into a whole-step graph read instead of kernel arguments. (The clip finalize kernel reads the
        gradient scale from slot 2 of a [4] tensor of its own, filled by the same copy.)"""
        if self.dcoef is None:
            both = torch.zeros(12, dtype=torch.float32, device=self.store.master.device)
            self.dcoef, self._dclip = both[:8], both[8:]
            self._dboth = both
        return self.dcoef

    def prepare_device_step(self, grad_scale: float) -> None:
        self._no_step_in_swap()
        self.step_count += 1
        ibc1, ibc2 = self._coeffs()
        self._fix_ema_w()
        gs = float(grad_scale)
        self._dboth.copy_(torch.tensor([self.lr, ibc1, ibc2, self.eps, gs, self.weight_decay, self._ema_w, 0.0,
                                        0.0, 0.0, gs, 0.0], dtype=torch.float32), non_blocking=True)

    # -------------------------------------------------------------------------- overlap with backward
    def enable_overlap(self, ranges, on_ready=None) -> None:
        super().enable_overlap(ranges, on_ready)
        # each slice as a run of whole segments (the tiles are anchored per segment, so a slice's launches write the
        # same bits a whole-buffer launch writes)
        offs = [s.offset for s in self.store.segments]
        ends = [o + sp for o, sp in zip(offs, self._spans)]
        self._seg_ranges = []
        for st, e in self._ranges:
            idx = [i for i, o in enumerate(offs) if st <= o < e]
            if not idx or offs[idx[0]] != st or ends[idx[-1]] > e or idx != list(range(idx[0], idx[-1] + 1)):
                raise ValueError(f"FusedLamb: slice [{st}, {e}) does not hold whole segments")
            self._seg_ranges.append((idx[0], len(idx)))

    def _launch(self, seg0: int, nsegs: int, ibc1: float, ibc2: float, gscale: float, zero_grad: bool,
                clip: Optional[torch.Tensor] = None) -> None:
        from ..ops import hip

        s = self.store
        out, out_lo = s.adam_outputs(0, s.numel)
        hip.lamb_step(self._plan, seg0, nsegs, s.master, self.exp_avg, self.exp_avg_sq, s.grad, out, out_lo,
                      self._partials, self._ratio, self.lr, ibc1, ibc2, self.eps, self.beta1, self.beta2, gscale,
                      self.weight_decay, self._kernel_coef(), clip, zero_grad, lr_mul=self._lr_mul, **self._ema_kw())

    @torch.no_grad()
    def step_range(self, b: int) -> None:
        """LAMB on slice ``b`` on the CURRENT stream, then the slice's Wᵀ refresh and fp8 re-quantisation. With
        ``max_grad_norm``: the slice's sum of squares instead, as :meth:`FusedAdam.step_range`."""
        if not self._began or self._done[b]:
            return
        s = self.store
        if self._clip_out is not None:
            from ..ops import hip

            hip.grad_sumsq(s.grad[self._ranges[b][0]:self._ranges[b][1]], self._clip_partials, self._clip_bases[b])
            self._done[b] = True
            return
        ibc1, ibc2, gscale = self._coef
        self._launch(*self._seg_ranges[b], ibc1, ibc2, gscale, getattr(self, "_zero", False))
        if self._tsub is not None:
            s.refresh_transposed_subset(self._tsub[b])
        if self._f8sub is not None:
            s.refresh_fp8_subset(self._f8sub[b])
        self._done[b] = True

    def _clipped_step(self, nparts: int, ibc1: float, ibc2: float, gscale: float, zero_grad: bool) -> None:
        """Finish the norm from ``nparts`` partials, then LAMB over the whole buffer with the device-side clip
        coefficient, then the end-of-step weight-copy refresh (current stream)."""
        from ..ops import hip

        hip.grad_clip_finalize(self._clip_partials, nparts, gscale, self.max_grad_norm, self._clip_out,
                               self._dclip if self._capturing else None)
        self._launch(0, len(self.store.segments), ibc1, ibc2, gscale, zero_grad, clip=self._clip_out[1:2])
        self.store.refresh_transposed()

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, zero_grad: bool = False) -> None:
        if getattr(self, "_began", False):
            self._finish_overlapped(grad_scale)
            return
        self._no_step_in_swap()
        self.step_count += 1
        ibc1, ibc2 = self._coeffs()
        self._fix_ema_w()
        s = self.store
        if s.master.is_cuda:
            from ..ops import hip

            hip.join_side_streams()  # weight gradients may still be in flight on the wgrad stream
            if self._clip_out is not None:
                n = hip.grad_sumsq(s.grad, self._clip_partials, 0)
                self._clipped_step(n, ibc1, ibc2, float(grad_scale), zero_grad)
                return
            self._launch(0, len(s.segments), ibc1, ibc2, float(grad_scale), zero_grad)
            s.refresh_transposed()
            return
        self._cpu_step(float(grad_scale), ibc1, ibc2)

    def _cpu_step(self, grad_scale: float, ibc1: float, ibc2: float) -> None:
        """Reference path: the same math with torch ops per segment, norms in fp64."""
        s = self.store
        g = s.grad.to(torch.float32)
        if self._clip_out is not None:
            # FusedAdam's CPU formula: norm in fp64, coef and grad_scale * coef rounded to fp32
            gs32 = torch.tensor(grad_scale, dtype=torch.float32)
            norm = math.sqrt(float(g.double().square().sum()) * float(gs32) ** 2)
            coef = self.max_grad_norm / norm if norm > self.max_grad_norm else 1.0
            self._clip_out[0], self._clip_out[1] = norm, coef
            grad_scale = float(gs32 * self._clip_out[1])
        g = g * grad_scale
        self.exp_avg.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
        self.exp_avg_sq.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
        for i, seg in enumerate(s.segments):
            sl = slice(seg.offset, seg.offset + seg.numel)
            w = s.master[sl]
            u = (self.exp_avg[sl] * ibc1) / ((self.exp_avg_sq[sl] * ibc2).sqrt() + self.eps)
            r = 1.0
            if seg.decay:
                if self.weight_decay:
                    u = u + self.weight_decay * w
                wn, un = float(w.double().square().sum().sqrt()), float(u.double().square().sum().sqrt())
                if wn > 0.0 and un > 0.0:  # a NaN norm compares false: r = 1
                    r = wn / un
            self._ratio[i, 0] = r
            lr = torch.tensor(self.lr, dtype=torch.float32)
            if self._mu is not None:
                lr = lr * self._mu[i]  # the kernel's rounding: fp32 lr times the fp32 multiplier, then times r
            w.sub_(u * float(lr * self._ratio[i, 0]))
        self._ema_cpu_update()
        if s.compute is not s.master:
            s.compute.copy_(s.master)
