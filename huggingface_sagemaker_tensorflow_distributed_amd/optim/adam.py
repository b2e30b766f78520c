"""Fused Adam / AdamW over the flat parameter store — one kernel launch per step.

Reference optimizer: ``tf.keras.optimizers.Adam(learning_rate)`` (``scripts/train.py:113``,
``scripts/singe_node_train.py:78``) — TF 2.4 Keras defaults β1=0.9, β2=0.999, ε=1e-7, no weight decay,
and the ε-hat update::

    lr_t = lr·√(1-β2ᵗ)/(1-β1ᵗ);  m = β1 m + (1-β1) g;  v = β2 v + (1-β2) g²;  θ -= lr_t·m/(√v + ε)

PyTorch's form divides √v by √(1-β2ᵗ) before adding ε; both are ``θ -= step·m/(√v + ε_eff)`` with
``ε_eff = ε`` (keras) or ``ε·√(1-β2ᵗ)`` (torch), so one kernel serves both (``eps_mode``).
The DP ``1/N`` gradient average (``hvd.DistributedOptimizer`` semantics) and the optional
gradient-accumulation ``1/k`` are folded into ``grad_scale``; with bf16 compute the kernel also
writes the bf16 weight copy the next forward reads (no separate cast pass).

Overlap with backward (:meth:`FusedAdam.enable_overlap`): the update is elementwise, so a contiguous slice of the
flat buffers can be stepped as soon as its gradients are final. The store is laid out in backward order, so
the slices complete front-to-back while the rest of backward still runs: one process runs each slice's Adam on
a side stream the moment its last gradient is queued; data-parallel ranks run it on the RCCL engine's stream
right after the slice's bucket all-reduce. The memory-bound update then shares the GPU with the compute-bound
backward GEMMs instead of following them (the bert-large optimizer pass moves ~10 GB per step). What is left
at ``step()`` is the join, the slices no gradient reached, and the batched Wᵀ refresh.

Global-norm clipping (``max_grad_norm=C > 0``; ``tf.clip_by_global_norm``, the math of Keras ``global_clipnorm``, no
epsilon): with ``g`` the gradient averaged over ranks and accumulation micro-steps, ``coef = C / ‖g‖₂`` if ``‖g‖₂ > C``
else 1, and Adam consumes ``coef · g``. Exact clipping needs the whole norm before any weight moves, so in clip mode
the overlap hooks run each slice's sum of squares under the backward instead of its update, and ``step()`` finishes
the norm on the device (no host round trip: a captured whole-step graph replays it) and runs ONE Adam over the whole
buffer that reads the coefficient from device memory. Data-parallel ranks take the norm over the all-reduced buffer,
which holds the same values on every rank (also with a bf16 / fp16 wire: every rank casts back the same reduced
values), so they agree on ``coef`` bit for bit without another collective.

Per-parameter learning rates (``lr_multipliers``; ``--layerwise_lr_decay`` / ``--head_lr_multiplier``, optim/groups.py):
every segment has a multiplier ``μ > 0`` and is stepped with ``lr·μ`` in both places the learning rate appears,
``θ = θ·(1 - (lr·wd)·μ·mask) - (step·μ)·m/(√v + ε)``; ``m`` and ``v`` do not see it. ``μ`` is rounded to fp32 once and
the kernel scales ``step`` and ``lr·wd`` by ONE fp32 multiply each, reading ``μ`` from an fp32 table with one entry per
64-element block (:meth:`FlatParamStore.block_table`), so a segment gets the bits of a step on that segment alone with
``float32(step·μ)`` and ``float32(lr·wd·μ)``. The schedule keeps scaling :attr:`lr`; ``μ`` multiplies whatever it is
at that step. ``None`` or all ones is off: no table, the launches without it.

Weight averaging (``ema_decay=d``, ``0 < d < 1``; ``--ema_decay`` / ``--ema_warmup``; Keras ``use_ema``, timm's
``ModelEmaV2``): one more fp32 buffer :attr:`ema`, laid out as ``store.master`` and starting as a bit copy of it. After
optimizer step ``t`` (0 for the first update; one per optimizer step, not per accumulation micro-step), with ``θ`` the
weight that step wrote, ``ema ← ema + ω_t·(θ − ema)`` as three separately rounded fp32 operations (subtract, multiply,
add: never an FMA -- a torch fp32 replay ``e + w * (p - e)`` gives the same bits). ``ω_t = float32(1 − d_t)`` with
``d_t = d``, or with ``ema_warmup`` ``d_t = min(d, (1 + t)/(10 + t))`` (``tf.train.ExponentialMovingAverage``'s
``num_updates`` rule), both formed in Python floats and rounded once. The update kernel does it in the pass that writes
``θ`` (one more 16-B load and store per chunk), so it rides every launch path the step has: slices under the backward,
the clipped whole-buffer pass, captured steps (``ω`` in :attr:`dcoef` slot 4). Nothing else reads :attr:`ema`: a step
with averaging on writes the bits of a step without it everywhere else. Ranks need no collective: the average is a
function of weights that are identical on every rank. :meth:`FusedAdam.ema_weights` exchanges the average into the
store for evaluation and saving. In fp32 the average stops moving where ``ω·(θ − ema)`` falls under half an ulp of
``ema``, as every fp32 EMA does. 0 is off: nothing is allocated, the launches without it.
"""
from __future__ import annotations

import contextlib
import logging
import math
import os
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from ..parallel.flat_params import ALIGN, FlatParamStore

logger = logging.getLogger(__name__)


class FusedAdam:
    # overlapped steps re-quantise each slice's fp8 weights right after its update (False: one pass at the end; A/B)
    per_slice_fp8 = True
    kind = "adam"  # what load_state_dict accepts (a state without a "kind" is Adam's)

    def __init__(self, store: FlatParamStore, lr: float = 1e-3, betas=(0.9, 0.999), eps: Optional[float] = None,
                 weight_decay: float = 0.0, eps_mode: str = "keras", decoupled: bool = True,
                 max_grad_norm: float = 0.0, lr_multipliers=None, ema_decay: float = 0.0, ema_warmup: bool = False):
        if eps_mode not in ("keras", "torch"):
            raise ValueError(eps_mode)
        if not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0 (0 = off, inf = report the norm only): {max_grad_norm!r}")
        self.store = store
        self.lr = float(lr)
        self.beta1, self.beta2 = map(float, betas)
        self.eps = float(eps if eps is not None else (1e-7 if eps_mode == "keras" else 1e-8))
        self.eps_mode = eps_mode
        self.weight_decay = float(weight_decay)
        self.decoupled = decoupled
        self.step_count = 0
        self.exp_avg = torch.zeros_like(store.master)
        self.exp_avg_sq = torch.zeros_like(store.master)
        self._decay_mask = store.decay_block_mask(ALIGN) if weight_decay else None
        self.dcoef: Optional[torch.Tensor] = None  # device-side step scalars (HIP-graph replays), see use_device_coef
        self._capturing = False  # dcoef is handed to the kernel only while a whole-step graph is being captured
        # global-norm clipping: [norm, coef] of the last step and the per-block partial sums of squares, on the device
        # at addresses that stay put (a captured graph replays the launches that read and write them). On or off is
        # fixed here; the value of C may change between eager steps (it travels as a kernel argument)
        self.max_grad_norm = float(max_grad_norm)
        self._clip_out: Optional[torch.Tensor] = None
        self._clip_partials: Optional[torch.Tensor] = None
        self._clip_bases: List[int] = []  # first partial slot of each overlap slice
        self._clip_nparts = 0
        if self.max_grad_norm > 0.0:
            self._clip_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=store.master.device)
            self._plan_clip([])
        # per-parameter learning-rate multipliers: fp32, one per segment (None = off), and the device table the kernels
        # read, built once at an address that stays put (captured graphs replay launches that read it)
        self._mu = self._resolve_multipliers(lr_multipliers)
        self._lr_mul: Optional[torch.Tensor] = None
        self._mu_elem: Optional[torch.Tensor] = None  # CPU path: the multiplier of every element
        if self._mu is not None:
            self._build_lr_table()
        # weight averaging: the decay (0 = off), the warm-up rule, and the average itself, allocated once at an address
        # that stays put (captured graphs replay launches that write it; ema_weights exchanges contents, never tensors)
        self.ema_decay = float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if self.ema_decay != 0.0 and not (0.0 < self.ema_decay < 1.0):  # NaN and inf fail the comparison
            raise ValueError(f"ema_decay must be 0 (off) or finite with 0 < d < 1: {ema_decay!r}")
        if self.ema_warmup and self.ema_decay == 0.0:
            raise ValueError("ema_warmup needs ema_decay > 0")
        self.ema: Optional[torch.Tensor] = None
        self._ema_w = 0.0  # this step's 1 - d_t (begin_step / step / prepare_device_step fix it)
        self._ema_swapped = False
        if self.ema_decay > 0.0:
            self.ema = torch.empty_like(store.master)
            self.reset_ema()

    # -------------------------------------------------------------------------- weight averaging
    def ema_decay_at(self, t: int) -> float:
        """``d_t`` of optimizer step ``t`` (0 = the first update): ``d``, or ``min(d, (1 + t)/(10 + t))`` with
        warm-up. A Python float; the step uses ``float32(1 - d_t)``."""
        d = self.ema_decay
        if self.ema_warmup:
            d = min(d, (1.0 + t) / (10.0 + t))
        return d

    def _fix_ema_w(self) -> None:
        """This step's ``ω`` (call after :attr:`step_count` advanced: step ``t = step_count - 1``)."""
        if self.ema is not None:
            self._ema_w = 1.0 - self.ema_decay_at(self.step_count - 1)

    def _ema_kw(self, st: Optional[int] = None, e: Optional[int] = None) -> dict:
        """The ``ema`` / ``ema_omd`` keywords of a launch on slice ``[st, e)`` (the whole buffer by default); empty
        when off, so the launch is the one made without the feature."""
        if self.ema is None:
            return {}
        return {"ema": self.ema if st is None else self.ema[st:e], "ema_omd": self._ema_w}

    def _ema_cpu_update(self) -> None:
        """CPU path: the kernel's three rounded fp32 operations after the weight update."""
        if self.ema is not None:
            d = self.store.master - self.ema
            d.mul_(torch.tensor(self._ema_w, dtype=torch.float32))
            self.ema.add_(d)

    @torch.no_grad()
    def reset_ema(self) -> None:
        """Restart the average from the current master weights (a bit copy): at construction, after the start-up
        broadcast of a fresh run, and on a resume from a checkpoint that carries no average."""
        if self.ema is not None:
            self.ema.copy_(self.store.master)

    def ema_state(self) -> Optional[Dict[str, torch.Tensor]]:
        """``{segment name: view of the average}`` shaped as the parameters; None when off."""
        if self.ema is None:
            return None
        return {sg.name: self.ema[sg.offset:sg.offset + sg.numel].view(sg.shape) for sg in self.store.segments}

    def _no_step_in_swap(self) -> None:
        if self._ema_swapped:
            raise RuntimeError("a training step inside ema_weights(): the store holds the averaged weights; leave the "
                               "context first")

    @contextlib.contextmanager
    def ema_weights(self):
        """Scope in which the store holds the averaged weights (evaluation, saving): the CONTENTS of ``master`` and
        :attr:`ema` are exchanged in place -- no tensor is rebound, captured eval graphs and parameter views point at
        these addresses -- and the bf16 copy, the Wᵀ / fp8 copies and the hi / lo halves are refreshed from them. On
        exit the contents are exchanged back and the copies restored, every buffer to the bits it held on entry (the
        fp8 copies, their scales and the activation amax history from a snapshot: re-quantising rolls that history).
        ``m``, ``v`` and the step count are never touched. A training step inside the scope raises."""
        if self.ema is None:
            raise RuntimeError("ema_weights(): construct the optimizer with ema_decay > 0")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is already active")
        if getattr(self, "_began", False):
            raise RuntimeError("ema_weights() inside an optimizer step (between begin_step and step)")
        s = self.store
        fp8 = [getattr(s, n) for n in ("fp8_w", "fp8_wt", "fp8_amax", "fp8_sinv", "fp8_act")] \
            if getattr(s, "_fp8_desc", None) is not None else []
        snap = [t.clone() for t in fp8]
        self._exchange_ema()
        s.sync_compute_from_master()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            self._exchange_ema()
            s.sync_compute_from_master()
            for t, c in zip(fp8, snap):
                t.copy_(c)

    _EXCHANGE_CHUNK = 1 << 24  # elements per chunk of the in-place exchange: a 64 MB temporary, whatever the model

    @torch.no_grad()
    def _exchange_ema(self) -> None:
        """Exchange the contents of ``master`` and :attr:`ema` in place, chunk by chunk through one small temporary."""
        a, b = self.store.master, self.ema
        tmp = torch.empty(min(self._EXCHANGE_CHUNK, a.numel()), dtype=a.dtype, device=a.device)
        for st in range(0, a.numel(), tmp.numel()):
            e = min(st + tmp.numel(), a.numel())
            t = tmp[:e - st]
            t.copy_(a[st:e])
            a[st:e].copy_(b[st:e])
            b[st:e].copy_(t)

    # -------------------------------------------------------------------------- per-parameter learning rates
    def _resolve_multipliers(self, given) -> Optional[torch.Tensor]:
        """``given`` ({segment name: μ} or a sequence in segment order) as an fp32 tensor [segments]; None when it is
        None or all ones."""
        if given is None:
            return None
        names = self.store.names
        if isinstance(given, dict):
            missing = [n for n in names if n not in given]
            if missing:
                raise ValueError(f"lr_multipliers: no multiplier for {len(missing)} segment(s), e.g. {missing[:3]}")
            vals = [float(given[n]) for n in names]
        else:
            vals = [float(x) for x in given]
            if len(vals) != len(names):
                raise ValueError(f"lr_multipliers: {len(vals)} values for {len(names)} segments")
        mu = torch.tensor(vals, dtype=torch.float64).to(torch.float32)  # rounded to fp32 once
        bad = [n for n, x in zip(names, mu.tolist()) if not (x > 0.0 and math.isfinite(x))]
        if bad:
            raise ValueError(f"lr_multipliers must be finite and > 0 in fp32 (freezing is not supported): {bad[:3]}")
        return None if bool((mu == 1.0).all()) else mu

    def _build_lr_table(self) -> None:
        """Adam's table: one fp32 entry per 64-element block (alignment padding and the tail hold 1)."""
        self._lr_mul = self.store.block_table(self._mu.tolist(), ALIGN)

    def _lr_mul_slice(self, st: int, e: int) -> Optional[torch.Tensor]:
        return self._lr_mul[st // ALIGN:(e + ALIGN - 1) // ALIGN] if self._lr_mul is not None else None

    def lr_multipliers(self) -> Optional[Dict[str, float]]:
        """``{segment name: μ}`` (the fp32 values the step uses), or None when off."""
        return dict(zip(self.store.names, self._mu.tolist())) if self._mu is not None else None

    # -------------------------------------------------------------------------- global-norm clipping
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Device scalar: the global norm of the last step's (averaged) gradient; None with clipping off."""
        return self._clip_out[0] if self._clip_out is not None else None

    @property
    def last_clip_coef(self) -> Optional[torch.Tensor]:
        """Device scalar: the factor the last step's gradient was scaled by (1 = not clipped)."""
        return self._clip_out[1] if self._clip_out is not None else None

    def grad_norm(self) -> float:
        """The global gradient norm of the last step, as a float. Synchronises with the device: call it only when
        logging. Needs ``max_grad_norm > 0`` (``inf`` measures the norm and never clips)."""
        if self._clip_out is None:
            raise RuntimeError("FusedAdam.grad_norm(): construct with max_grad_norm > 0 (inf = report only)")
        return float(self._clip_out[0].item())

    def _plan_clip(self, ranges) -> None:
        """Partial-sum slots of the overlap slices ``ranges`` (the whole buffer as one slice always fits too)."""
        s = self.store
        if self._clip_out is None or not s.master.is_cuda:
            return
        from ..ops import hip

        bf = s.grad.dtype == torch.bfloat16
        self._clip_bases, n = [], 0
        for st, e in ranges:
            self._clip_bases.append(n)
            n += hip.grad_sumsq_blocks(e - st, bf)
        self._clip_nparts = n
        need = max(n, hip.grad_sumsq_blocks(s.numel, bf))
        if self._clip_partials is None or self._clip_partials.numel() < need:
            self._clip_partials = torch.zeros(need, dtype=torch.float32, device=s.master.device)

    def _clipped_step(self, nparts: int, step: float, eps_eff: float, gscale: float, zero_grad: bool) -> None:
        """Finish the norm from ``nparts`` partials, then ONE Adam over the whole buffer with the device-side clip
        coefficient, then the end-of-step weight-copy refresh (current stream)."""
        from ..ops import hip

        s = self.store
        hip.grad_clip_finalize(self._clip_partials, nparts, gscale, self.max_grad_norm, self._clip_out,
                               self._kernel_coef())
        out, out_lo = s.adam_outputs(0, s.numel)
        hip.adam_step(s.master, self.exp_avg, self.exp_avg_sq, s.grad, out, self._decay_mask, step, eps_eff,
                      self.beta1, self.beta2, gscale, self.lr * self.weight_decay, self._kernel_coef(), out_lo,
                      zero_grad=zero_grad, clip=self._clip_out[1:2], lr_mul=self._lr_mul, **self._ema_kw())
        s.refresh_transposed()

    # --------------------------------------------------------------------------
    def state_tensors(self) -> List[torch.Tensor]:
        return [self.exp_avg, self.exp_avg_sq] + ([self.ema] if self.ema is not None else [])

    def state_dict(self) -> dict:
        sd = {"step": self.step_count, "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
              "lr": self.lr, "betas": (self.beta1, self.beta2), "eps": self.eps, "eps_mode": self.eps_mode,
              "weight_decay": self.weight_decay}
        if self._mu is not None:
            sd["lr_multipliers"] = self.lr_multipliers()
        if self.ema is not None:
            sd["ema"] = self.ema.cpu()
            sd["ema_decay"] = self.ema_decay
            sd["ema_warmup"] = self.ema_warmup
        return sd

    def load_state_dict(self, sd: dict) -> None:
        # states of other optimizers over the same buffers (optim/lamb.py) carry their "kind"; Adam's own carry none
        kind = sd.get("kind")
        if kind is not None and kind != self.kind:
            raise ValueError(f"optimizer state of kind {kind!r} cannot be loaded into {type(self).__name__} "
                             f"(kind {self.kind!r}): resume with the --optimizer the checkpoint was written with")
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"].to(self.exp_avg.device))
        self.exp_avg_sq.copy_(sd["exp_avg_sq"].to(self.exp_avg_sq.device))
        was = sd.get("lr_multipliers")
        if was is not None and all(float(x) == 1.0 for x in was.values()):
            was = None
        if was != self.lr_multipliers():
            logger.warning("the checkpoint was written with %s and this optimizer runs with %s: the current "
                           "--layerwise_lr_decay / --head_lr_multiplier win", _describe_mul(was),
                           _describe_mul(self.lr_multipliers()))
        was_ema = (float(sd.get("ema_decay", 0.0)), bool(sd.get("ema_warmup", False)))
        if was_ema != (self.ema_decay, self.ema_warmup):
            logger.warning("the checkpoint was written with %s and this optimizer runs with %s: the current "
                           "--ema_decay / --ema_warmup win", _describe_ema(*was_ema),
                           _describe_ema(self.ema_decay, self.ema_warmup))
        if self.ema is not None:
            if sd.get("ema") is not None:
                self.ema.copy_(sd["ema"].to(self.ema.device))
            else:
                logger.warning("the checkpoint carries no weight average: the average restarts from the loaded "
                               "weights")
                self.reset_ema()

    def _coeffs(self):
        t = self.step_count
        bc1 = 1.0 - self.beta1 ** t
        bc2 = 1.0 - self.beta2 ** t
        step = self.lr * math.sqrt(bc2) / bc1
        eps_eff = self.eps if self.eps_mode == "keras" else self.eps * math.sqrt(bc2)
        return step, eps_eff

    # -------------------------------------------------------------------------- device-side coefficients
    def use_device_coef(self) -> torch.Tensor:
        """The fp32 [8] device tensor (step, eps, grad_scale, lr*wd, 1 - ema decay, -, -, -) that Adam launches
        CAPTURED into a HIP graph of the whole training step read instead of kernel arguments, so replays run with
        each step's bias correction, learning rate and averaging weight (train/graph.py). :meth:`prepare_device_step`
        fills it before a replay. Only launches issued inside :meth:`capturing` read it; eager steps always pass their
        own scalars."""
        if self.dcoef is None:
            self.dcoef = torch.zeros(8, dtype=torch.float32, device=self.store.master.device)
        return self.dcoef

    @contextlib.contextmanager
    def capturing(self):
        """Scope of a whole-step graph capture: Adam launches inside it take their scalars from :attr:`dcoef`."""
        self.use_device_coef()
        self._capturing = True
        try:
            yield
        finally:
            self._capturing = False

    def _kernel_coef(self) -> Optional[torch.Tensor]:
        return self.dcoef if self._capturing else None

    def prepare_device_step(self, grad_scale: float) -> None:
        """Advance the step count and write this step's scalars to :attr:`dcoef` (stream-ordered H2D copy of a
        fresh host tensor: the host may move on at once)."""
        self._no_step_in_swap()
        self.step_count += 1
        step, eps_eff = self._coeffs()
        self._fix_ema_w()
        self.dcoef.copy_(torch.tensor([step, eps_eff, float(grad_scale), self.lr * self.weight_decay, self._ema_w,
                                       0.0, 0.0, 0.0], dtype=torch.float32), non_blocking=True)

    # -------------------------------------------------------------------------- overlap with backward
    def enable_overlap(self, ranges: List[Tuple[int, int]], on_ready: Optional[Callable] = None) -> None:
        """Step the flat-buffer slices ``ranges`` (64-aligned, backward order) as their gradients complete.

        INVARIANT (the overlap is correct only under it): every kernel that READS a parameter -- its bf16 copy, its
        Wᵀ / fp8 copies -- is queued before that parameter's post-accumulate hook fires. Autograd runs the hook after
        the last node that used the parameter, and the HIP backward kernels read weights inside those nodes, so this
        holds for the model code here; it would NOT hold for activation recompute (a re-run forward reads weights
        after their hook) or a head that reads weights outside autograd after the hook. A model that breaks it sets
        ``opt_overlap_safe = False`` and the Trainer then steps the optimizer once after backward.

        ``on_ready``: the store-readiness callback to install (one process); data-parallel ranks call
        :meth:`step_range` from the bucketer instead."""
        self._ranges = list(ranges)
        self._done = [False] * len(self._ranges)
        self._began = False
        self._plan_clip(self._ranges)
        # each slice's Wᵀ copies are refreshed right after its update (fp8 weight copies, which need the whole
        # step's amax, are still re-quantised once at the end)
        self._tsub = self.store.transposed_subsets(self._ranges) if self.store.master.is_cuda else None
        # ... and each slice's fp8 weight copies right after that (fp8 runs): the per-weight amax / quantise passes
        # leave the end of the step, where they ran alone (~0.5 ms per roberta-large step)
        self._f8sub = self.store.fp8_subsets(self._ranges) if self._tsub is not None and self.per_slice_fp8 else None
        if on_ready is not None:
            self.store.ready_callback = on_ready

    @property
    def overlap_enabled(self) -> bool:
        return bool(getattr(self, "_ranges", None))

    def begin_step(self, grad_scale: float, zero_grad: bool = False) -> None:
        """Fix this step's coefficients before backward (the slices are stepped during it). ``zero_grad``: each slice's
        Adam also clears the gradients it read (:meth:`step`)."""
        self._no_step_in_swap()
        self.step_count += 1
        step, eps_eff = self._coeffs()
        self._fix_ema_w()
        self._coef = (step, eps_eff, float(grad_scale))
        self._zero = bool(zero_grad) and self.store.grad.is_cuda
        self._done = [False] * len(self._ranges)
        self._began = True

    def abort_step(self) -> None:
        """Undo :meth:`begin_step` when the step fails before :meth:`step` (an exception in backward, an OOM at an
        auto-planned batch): the bias-correction step count must not drift by one per failed step. Slices already
        stepped under the failed backward cannot be undone; the caller is expected to stop or restore a checkpoint."""
        if getattr(self, "_began", False):
            self.step_count -= 1
            self._began = False

    @torch.no_grad()
    def step_range(self, b: int) -> None:
        """Adam on slice ``b`` on the CURRENT stream (the caller orders it after the slice's gradients). With
        ``max_grad_norm``: the slice's sum of squares instead -- no weight may move before the whole norm is known;
        the update (and the Wᵀ / fp8 refresh) is one pass at :meth:`step`."""
        if not self._began or self._done[b]:
            return
        from ..ops import hip

        st, e = self._ranges[b]
        s = self.store
        if self._clip_out is not None:
            hip.grad_sumsq(s.grad[st:e], self._clip_partials, self._clip_bases[b])
            self._done[b] = True
            return
        step, eps_eff, gscale = self._coef
        out, out_lo = s.adam_outputs(st, e)
        dm = self._decay_mask[st // ALIGN:(e + ALIGN - 1) // ALIGN] if self._decay_mask is not None else None
        hip.adam_step(s.master[st:e], self.exp_avg[st:e], self.exp_avg_sq[st:e], s.grad[st:e], out, dm, step,
                      eps_eff, self.beta1, self.beta2, gscale, self.lr * self.weight_decay, self._kernel_coef(), out_lo,
                      zero_grad=getattr(self, "_zero", False), lr_mul=self._lr_mul_slice(st, e), **self._ema_kw(st, e))
        if self._tsub is not None:
            s.refresh_transposed_subset(self._tsub[b])
        if self._f8sub is not None:
            s.refresh_fp8_subset(self._f8sub[b])
        self._done[b] = True

    @torch.no_grad()
    def _finish_overlapped(self, grad_scale: float) -> None:
        from ..ops import hip

        if abs(grad_scale - self._coef[2]) > 1e-12 * max(1.0, abs(grad_scale)):
            raise RuntimeError("FusedAdam: grad_scale changed between begin_step and step")
        hip.join_side_streams()
        for b in range(len(self._ranges)):  # slices no gradient reached (unused parameters)
            self.step_range(b)
        self._began = False
        zero, self._zero = getattr(self, "_zero", False), False
        if self._clip_out is not None:
            # every slice's partials were rewritten this step (under the backward, or just above)
            self._clipped_step(self._clip_nparts, self._coef[0], self._coef[1], self._coef[2], zero)
            return
        if self._tsub is None:
            self.store.refresh_transposed()
        elif self._f8sub is not None:
            self.store.finish_fp8_step()
        else:
            self.store.refresh_fp8()

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, zero_grad: bool = False) -> None:
        """``zero_grad`` (GPU): the kernel clears each gradient after reading it, so the caller (the Trainer) can skip
        its next :meth:`FlatParamStore.zero_grad` -- the memset pass over the whole gradient buffer moves into the
        optimizer's own pass (which, overlapped with backward, runs under the weight-gradient GEMMs). With the overlap,
        :meth:`begin_step` decides it."""
        if getattr(self, "_began", False):
            self._finish_overlapped(grad_scale)
            return
        self._no_step_in_swap()
        self.step_count += 1
        step, eps_eff = self._coeffs()
        self._fix_ema_w()
        s = self.store
        write_compute = s.compute is not s.master
        if s.master.is_cuda:
            from ..ops import hip

            hip.join_side_streams()  # weight gradients may still be in flight on the wgrad stream
            if self._clip_out is not None:
                n = hip.grad_sumsq(s.grad, self._clip_partials, 0)
                self._clipped_step(n, step, eps_eff, float(grad_scale), zero_grad)
                return
            out, out_lo = s.adam_outputs(0, s.numel)
            hip.adam_step(s.master, self.exp_avg, self.exp_avg_sq, s.grad, out,
                          self._decay_mask, step, eps_eff, self.beta1, self.beta2, float(grad_scale),
                          self.lr * self.weight_decay, self._kernel_coef(), out_lo, zero_grad=zero_grad,
                          lr_mul=self._lr_mul, **self._ema_kw())
            s.refresh_transposed()
            return
        # reference path (CPU): identical math on flat buffers
        g = s.grad.to(torch.float32)
        if self._clip_out is not None:
            # the GPU path's formula: norm in fp64, coef and grad_scale * coef rounded to fp32
            gs32 = torch.tensor(float(grad_scale), dtype=torch.float32)
            norm = math.sqrt(float(g.double().square().sum()) * float(gs32) ** 2)
            coef = self.max_grad_norm / norm if norm > self.max_grad_norm else 1.0
            self._clip_out[0], self._clip_out[1] = norm, coef
            grad_scale = float(gs32 * self._clip_out[1])
        g = g * grad_scale
        mu = None
        if self._mu is not None:
            # the kernel's rounding: step and lr * wd as fp32 scalars, each times the element's fp32 multiplier
            if self._mu_elem is None:
                self._mu_elem = self._lr_mul.repeat_interleave(ALIGN)[: s.numel]
            mu = self._mu_elem
        if self.weight_decay:
            wd = self._decay_mask.repeat_interleave(ALIGN)[: s.numel].to(torch.float32)
            if mu is None:
                s.master.mul_(1.0 - self.lr * self.weight_decay * wd)
            else:
                s.master.mul_(1.0 - torch.tensor(self.lr * self.weight_decay, dtype=torch.float32) * mu * wd)
        self.exp_avg.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
        self.exp_avg_sq.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
        if mu is None:
            s.master.addcdiv_(self.exp_avg, self.exp_avg_sq.sqrt().add_(eps_eff), value=-step)
        else:
            s.master.sub_((torch.tensor(step, dtype=torch.float32) * mu) * self.exp_avg
                          / self.exp_avg_sq.sqrt().add_(eps_eff))
        self._ema_cpu_update()
        if write_compute:
            s.compute.copy_(s.master)


def _describe_mul(mul: Optional[Dict[str, float]]) -> str:
    if mul is None:
        return "no learning-rate multipliers"
    v = list(mul.values())
    return f"learning-rate multipliers in [{min(v):.6g}, {max(v):.6g}]"


def _describe_ema(decay: float, warmup: bool) -> str:
    return f"weight averaging at decay {decay:g}{' with warm-up' if warmup else ''}" if decay else "no weight averaging"


def plan_ranges(store: FlatParamStore, bucket_mb: float) -> Tuple[List[Tuple[int, int]], List[int]]:
    """Contiguous slices of ~``bucket_mb`` of gradients over whole segments, and each parameter's slice."""
    limit = int(bucket_mb * (1 << 20)) // store.grad.element_size()
    ranges, owner, start = [], [0] * len(store.segments), 0
    for i, _seg in enumerate(store.segments):
        owner[i] = len(ranges)
        end = store.segments[i + 1].offset if i + 1 < len(store.segments) else store.numel
        if end - start >= limit or i + 1 == len(store.segments):
            ranges.append((start, end))
            start = end
    return ranges, owner


class LocalOverlap:
    """One-process driver of :meth:`FusedAdam.enable_overlap`: counts each slice's ready gradients (the store's
    post-accumulate hooks) and, when the last one is queued, runs the slice's Adam on a side stream that first
    waits for everything queued so far on the compute (and wgrad) streams."""

    # False: every slice records its own event on the compute stream (the round-5 behaviour), for A/B runs
    defer_to_fork = True

    def __init__(self, opt: FusedAdam, bucket_mb: Optional[float] = None):
        store = opt.store
        # 16 MiB slices: bert-large S=512 B=8 +0.6 % over 32 (more of the optimizer under the backward), the headline
        # neutral (profiles/opt_slice_size_ab_r4.log)
        mb = bucket_mb if bucket_mb else float(os.environ.get("HSD_OPT_BUCKET_MB", "16"))
        self.ranges, self.owner = plan_ranges(store, mb)
        self.count = [0] * len(self.ranges)
        for o in self.owner:
            self.count[o] += 1
        self.pending = list(self.count)
        self.opt = opt
        self.stream = torch.cuda.Stream(device=store.device)
        self.sync = True
        # the stream the backward kernels are queued on, when it is not the hook thread's current stream: a HIP
        # graph capture (the capture stream; train/graph.py). Post-accumulate hooks of gradients the HIP backward
        # writes into main_grad itself run on autograd's thread with no producer stream (its current stream is the
        # device default), so a slice's fork must name the stream the gradients were really queued on.
        self.parent: Optional[torch.cuda.Stream] = None
        # contention emulation (tools/contention_ab.py): before each of the first HSD_HOG_POINTS slices of a step,
        # hold HSD_HOG_CUS whole CUs for HSD_HOG_US us on the slice stream -- what a data-parallel rank's RCCL
        # all-reduce kernels do beside its backward GEMMs -- so one GPU measures the persistent GEMMs under it
        self._hog = (int(os.environ.get("HSD_HOG_CUS", "0")), float(os.environ.get("HSD_HOG_US", "400")),
                     int(os.environ.get("HSD_HOG_POINTS", "7")))
        self._hogs = 0
        # slices whose gradients are final, waiting for the next weight-gradient fork (eager steps): a slice must
        # follow every compute-stream kernel that wrote its gradients or READ its weights (the block's last dgrad is
        # queued after the block's last fork), and the NEXT fork's side-stream position is after all of them. Ordering
        # the slice behind that position (an event recorded on the side stream) instead of recording an event on the
        # compute stream per slice takes ~3 us per slice off the compute stream's critical path (tools/fork_cost.py).
        self._deferred: List[int] = []
        self._forked = False  # a weight-gradient fork happened in this backward
        from ..ops import hip

        if self._on_fork not in hip._FORK_LISTENERS:
            hip._FORK_LISTENERS.append(self._on_fork)
        opt.enable_overlap(self.ranges, on_ready=self.mark_ready)

    def begin(self) -> None:
        self.pending = list(self.count)
        self.sync = True
        self._hogs = 0
        self._deferred = []
        self._forked = False

    def _launch(self, blocks: List[int]) -> None:
        with torch.cuda.stream(self.stream):
            for b in blocks:
                if self._hog[0] > 0 and self._hogs < self._hog[2]:
                    from ..ops import hip

                    self._hogs += 1
                    hip._C.cu_hog(self._hog[0], self._hog[1])
                self.opt.step_range(b)

    def _on_fork(self, side) -> None:
        """A weight-gradient fork just made ``side`` wait for the compute stream: the deferred slices follow it."""
        if side.device != self.stream.device:
            return
        self._forked = True
        if self._deferred:
            from ..ops import hip

            hip.stream_wait(self.stream, side)
            blocks, self._deferred = self._deferred, []
            self._launch(blocks)

    def mark_ready(self, i: int) -> None:
        if not self.sync:  # accumulation micro-step: gradients are not final yet
            return
        b = self.owner[i]
        self.pending[b] -= 1
        if self.pending[b] == 0:
            if self.parent is None and self._forked and self.defer_to_fork:
                self._deferred.append(b)  # launched behind the next weight-gradient fork (or at join)
                return
            from ..ops import hip

            cur = self.parent if self.parent is not None else torch.cuda.current_stream(self.stream.device)
            hip.stream_wait(self.stream, cur)
            side = hip.side_stream(self.stream.device)
            if side is not None and hip.side_stream_waitable():
                hip.stream_wait(self.stream, side)
            self._launch([b])

    def join(self) -> None:
        from ..ops import hip

        cur = torch.cuda.current_stream(self.stream.device)
        if self._deferred:
            # slices ready after the backward's last fork: behind the compute stream, which has joined the side
            # stream by now (Trainer.train_step joins the side streams before this)
            hip.stream_wait(self.stream, cur)
            blocks, self._deferred = self._deferred, []
            self._launch(blocks)
        self._forked = False
        hip.stream_wait(cur, self.stream)
