"""FusedAdamW: torch.optim.Optimizer whose step() is one multi-tensor HIP kernel sweep (ff_adamw_step) over all parameters
of a dtype — same update rule, defaults and state_dict layout (`step`, `exp_avg`, `exp_avg_sq`) as torch.optim.AdamW, so
optimizer checkpoints interchange.  The reference trains with `--optim adamw_torch` (training/train.sh:10-13) on
`model.parameters_trainable()`.

`capturable=True` keeps the step count AND the learning rate in device scalars per parameter group (bias corrections are computed
in the kernel), so `step()` can be captured into a HIP graph and replayed (graphs.GraphedTrainStep) while an LR scheduler keeps
changing `group["lr"]`: call `sync_device_hyperparams()` (GraphedTrainStep does) before a replay.  `state_dict()` reads the count back.

Mixed precision (the reference trains with `--fp16` autocast = fp32 master weights and fp32 moments, training/train.sh:24):
`master_dtype=torch.float32` keeps an fp32 master copy of every bf16 parameter in the optimizer state (`state["master"]`); the kernel
updates the master copy and writes its bf16 rounding into the parameter in the same pass, so steps far below the bf16 resolution of a
weight (lr 1e-4) accumulate instead of vanishing.  `state_dtype=torch.float32` alone keeps only the two moments in fp32.

Gradient clipping (the reference's HF Trainer clips the global L2 norm of the gradients to `max_grad_norm`, default 1.0, before every
step): `max_grad_norm=c` makes step() equal torch.nn.utils.clip_grad_norm_(params, c) followed by the AdamW update, without a pass that
rewrites the gradients - one sum-of-squares sweep over every gradient of every group (ff_grad_sumsq, fixed per-workgroup slots), an fp64
reduction to the norm and the coefficient on the device (ff_grad_sumsq_reduce, ff_grad_clip_coef), and the AdamW kernel multiplies each
gradient by the coefficient as it reads it (ff_adamw_step_clipped); `.grad` stays unscaled.  `grad_norm` is the pre-clip norm of the last
step (what HF logs as grad_norm), a device scalar that keeps its storage, so it is valid after a graph replay too.  Nothing synchronises
with the host: GraphedTrainStep captures the clipped step as it is.  With data parallelism, GradientAllReducer.finish() has averaged the
gradients before step() reads them, so the norm is the global one; ShardedAdamW takes its own max_grad_norm.

Gradient accumulation (the reference's recipe sets `--gradient_accumulation_steps`): `accumulate(scale)` after every micro-batch's backward
folds each `.grad` into an fp32 accumulator of the parameter's shape (ff_grad_accumulate: one fused multiply-add per element, the first
fold of a step overwrites, so nothing is zeroed) and sets `.grad = None`; the next `step()` takes the accumulators as the gradients
(ff_adamw_step_acc, the clip norm from ff_grad_sumsq over them).  Against autograd's own `grad += g`: the sum of bf16 gradients is kept in
fp32 instead of being rounded to 8 bits after every micro-batch, and because every backward finds `.grad is None` the gated blocks keep
their deferred, grouped weight-gradient launches in every micro-batch.  The accumulators cost 4 bytes per trainable parameter and live
outside `state`, so `state_dict()` stays torch.optim.AdamW's.  Nothing synchronises: graphs.GraphedTrainStep(micro_batches=k) captures
k x (forward, backward, accumulate(1 / k)) + step() as one graph.

Non-finite gradients (the reference trains with `--fp16` under HF Trainer's GradScaler, which does not take a step whose gradients hold an
inf or a NaN): `skip_nonfinite=True` (needs `capturable=True`) decides and skips on the device, so the guard works inside a replayed graph
where no host check can stand.  DEFINITION: a step is skipped iff the sum of squares of the (grad_scale'd) gradients - fp32 per workgroup,
fp64 in total, the sweep of clipping - is non-finite.  Squares are non-negative, so nothing cancels: every inf / NaN element is found, and
so are finite gradients so large that a 32768-element chunk's sum of squares overflows fp32 (a norm beyond about 1.8e19: garbage anyway).
step() always runs the sweep (ff_grad_sumsq over `.grad` or the open cycle's accumulators, ff_grad_sumsq_reduce), ff_grad_guard in the
place of ff_grad_clip_coef (norm, coefficient, `step_skipped`, the running `skipped_steps`; max_grad_norm is optional), advances the device
step counters by 1 - skipped, and updates every bucket with ff_adamw_step_guarded, whose workgroups return before touching a tensor when the
step is skipped: parameters, both moments, master copies and the step count stay bit for bit what they were, and the next taken step uses
the bias corrections of step t, not t + 1.  `.grad` is never modified; an accumulation cycle is closed after a skipped step too.  Graphed
steps capture it as they capture clipping; the loss a replay returns for a skipped step is that step's own, non-finite loss.  With
GradientAllReducer the averaged gradients are non-finite on every rank as soon as they are on one, so all ranks skip together.

torch.amp.GradScaler (eager): a capturable FusedAdamW sets `_step_supports_amp_scaling`, so `scaler.step(opt)` hands over its device scalars
`opt.found_inf` / `opt.grad_scale` and calls step() without a host round trip.  step() passes them to ff_grad_guard: the step is skipped on
found_inf != 0, the gradients are unscaled as they are read (coefficient / scale) - `.grad` keeps the scaled values, `grad_norm` is the norm
of the unscaled gradients.  The sweep runs only if skip_nonfinite or max_grad_norm asks for it.  Not with an open accumulate() cycle.

Stochastic rounding (pure-bf16 training without master copies): at the reference's lr 1e-4 an update is below half a bf16 ulp of most weights,
and a store that rounds to nearest drops it - a weight of 0.75 never moves, and bf16 moments stall the same way (stochastic
rounding).  `stochastic_rounding=True` stores every bf16 result of the kernel - the parameter, and the moments unless `state_dtype=torch.float32`
keeps them in fp32 - as one of its two bf16 neighbours with probability proportional to the distance (ff_adamw_step_sr), so every store is
unbiased and small updates accumulate in expectation: 4 bytes of optimizer state per parameter instead of the 12 of `master_dtype=torch.float32`,
which it excludes (a master copy already keeps the bits).  The random bits are a pure function of (`sr_seed`, the parameter's ordinal in
`param_groups` order, the step number, which of the three arrays, the element index) - Philox4x32-7, csrc/ff_sr.h - so two optimizers built
alike make the same decisions whatever the bucketing: on every data-parallel rank, under step(only=...) in any partition, with or without
accumulate(), eagerly or replayed from a graph; a skipped step does not consume its step number's bits.  Both settings are optimizer-wide and
stay out of state_dict() (`step` is in it: resuming with the same arguments continues the same streams).  fp32 parameters of the same optimizer
are updated as without it.

Exponential moving average of the weights (evaluating the Polyak average gives a better and steadier checkpoint than the last iterate):
`ema_decay=d` keeps an fp32 shadow of every parameter in the optimizer state (`state["ema"]`, created with the state as a copy of the weight
before its first update) and averages it on the device, one ff_ema_update after each bucket's AdamW launch on the same stream:
ema += (1 - d_t) (theta - ema), theta = the fp32 master copy where there is one, else the parameter; `ema_warmup=True` uses
d_t = min(d, (1 + t) / (10 + t)), `ema_every=k` averages on every k-th step only.  The launch reads the step count where the AdamW launch
reads it and the guard's verdict, so a captured step contains the averaging, and a step skipped on the device leaves every shadow bit for bit
and does not consume a warmup step.  step(only=...) averages exactly the parameters it updates.  DEVIATION from the textbook rule: a
parameter without a gradient in a step is not updated by this optimizer and is not averaged in that step either.  The shadow is always
fp32 (weight averaging: a bf16 shadow either never moves or carries the rounding noise of 1 / (1 - d) stores); with
`stochastic_rounding=True` it averages the rounding noise of the stored weights away, for 4 bytes per parameter.  The three settings are
optimizer-wide and stay out of state_dict(); the shadows are in it.  `ema_parameters()` yields (parameter, shadow) pairs;
`with opt.swap_ema():` puts the averages into the parameters IN PLACE (rounded to nearest in the parameter's dtype, the same storage: cached
decode sessions and captured graphs stay valid) and restores the weights bit for bit on exit."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Iterable, Optional

import torch

from . import ffi


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 grad_scale: float = 1.0, capturable: bool = False, master_dtype=None, state_dtype=None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, stochastic_rounding: bool = False, sr_seed: int = 0, ema_decay: Optional[float] = None,
                 ema_warmup: bool = False, ema_every: int = 1):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        if ema_decay is not None and not 0 < float(ema_decay) < 1:
            raise ValueError(f"ema_decay must be in (0, 1) (None: no averaging), got {ema_decay}")
        if int(ema_every) != ema_every or ema_every < 1:
            raise ValueError(f"ema_every must be an integer >= 1, got {ema_every}")
        if ema_decay is None and (ema_warmup or ema_every != 1):
            raise ValueError("ema_warmup / ema_every are settings of the weight average: they need ema_decay")
        # optimizer-wide and out of state_dict() as well; the shadows (state[p]["ema"]) are state
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup, self.ema_every = bool(ema_warmup), int(ema_every)
        self._ema_swapped = False                         # inside `with swap_ema()`: the parameters hold the averages
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be > 0 (None: no clipping), got {max_grad_norm}")
        # an optimizer-wide setting (the norm spans every group), so it is no group hyper-parameter and stays out of state_dict()
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip = None                                 # clipping: partials / fp64 sum / norm / coefficient on the device (first step)
        # optimizer-wide as well (one verdict per step) and out of state_dict(); the step count must live on the device to be conditional
        self.skip_nonfinite = bool(skip_nonfinite)
        if master_dtype not in (None, torch.float32) or state_dtype not in (None, torch.float32):
            raise ValueError("master_dtype / state_dtype: None (the parameter's dtype) or torch.float32")
        if master_dtype is not None:
            state_dtype = torch.float32                   # fp32 masters go with fp32 moments
        self.master_dtype, self.state_dtype = master_dtype, state_dtype
        # optimizer-wide and out of state_dict() as well: with `step`, which is in it, they name the random bits of every store
        self.stochastic_rounding, self.sr_seed = bool(stochastic_rounding), int(sr_seed)
        if self.stochastic_rounding and master_dtype is not None:
            raise ValueError("FusedAdamW(stochastic_rounding=True) is for bf16 parameters without master copies: not with master_dtype (an fp32 "
                             "master copy already keeps the bits a rounded store would drop)")
        if not 0 <= self.sr_seed < 2 ** 64:
            raise ValueError(f"sr_seed must be a 64-bit unsigned integer, got {sr_seed}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, capturable=capturable))
        self._acc = {}                                    # accumulate(): parameter -> its fp32 accumulator (kept from cycle to cycle)
        self._acc_fresh = set()                           # ... the parameters folded at least once since the last step()
        self._acc_open = False                            # ... a cycle is open: step() reads the accumulators
        if self.max_grad_norm is not None and len({p.device for g in self.param_groups for p in g["params"]}) > 1:
            raise ValueError("FusedAdamW(max_grad_norm=...) needs every parameter on one device (the global norm is reduced on it)")
        if self.skip_nonfinite and not all(g.get("capturable", False) for g in self.param_groups):
            raise ValueError("FusedAdamW(skip_nonfinite=True) needs capturable=True (a skipped step must not advance the step count, so the "
                             "count lives on the device)")
        if self.skip_nonfinite and len({p.device for g in self.param_groups for p in g["params"]}) > 1:
            raise ValueError("FusedAdamW(skip_nonfinite=True) needs every parameter on one device (the verdict is reached on it)")

    def add_param_group(self, param_group) -> None:
        """Every parameter gets its stochastic-rounding stream id here: its ordinal in param_groups order, never changed afterwards (the
        constructor adds the groups through this method)."""
        super().add_param_group(param_group)
        ids = self.__dict__.setdefault("_sr_ids", {})
        for p in self.param_groups[-1]["params"]:
            ids.setdefault(p, len(ids))
        if len(ids) > 2 ** 30:
            raise ValueError("FusedAdamW: more than 2^30 parameters (the stochastic-rounding stream id has 30 bits)")

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """max_grad_norm / skip_nonfinite: the total L2 norm of the gradients (grad_scale applied, a GradScaler's scale removed) BEFORE
        clipping, from the last step - a 0-dim fp32 device tensor whose storage is the same every step (None before the first step, and
        when no step computed a norm).  Non-finite for a skipped step."""
        return None if self._clip is None or not self._clip["swept"] else self._clip["norm"]

    @property
    def step_skipped(self) -> Optional[torch.Tensor]:
        """1 if the last step() was skipped for non-finite gradients, else 0: a 0-dim fp32 device tensor whose storage is the same every
        step (None before the first guarded step)."""
        return None if self._clip is None else self._clip["skip"]

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        """How many steps were skipped so far: a 0-dim int64 device tensor whose storage is the same every step (None before the first
        guarded step)."""
        return None if self._clip is None else self._clip["total"]

    @property
    def _step_supports_amp_scaling(self) -> bool:
        """torch.amp.GradScaler's protocol: True = GradScaler.step() sets `found_inf` / `grad_scale` (device scalars) on the optimizer and
        calls step(), which skips and unscales on the device.  Only when every group is capturable (a skipped step must not count);
        other optimizers keep GradScaler's generic path."""
        return all(g.get("capturable", False) for g in self.param_groups)

    @torch.no_grad()
    def accumulate(self, scale: float = 1.0) -> None:
        """Fold every `.grad` into the parameter's fp32 accumulator, acc = (first fold since the last step() ? 0 : acc) + scale * grad, and
        set `.grad = None` (one ff_grad_accumulate call per gradient dtype and device).  Opens an accumulation cycle: the next step() reads
        the accumulators.  Enqueues on the current stream only - no allocation after the first cycle, no synchronisation (capturable)."""
        from . import functional as _F
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.accumulate() inside `with swap_ema()`: the parameters hold the averaged weights")
        lib = ffi.lib()
        calls = {}
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                ffi.require_cuda(p, g)
                if g.dtype not in (torch.float32, torch.bfloat16) or not g.is_contiguous() or g.numel() != p.numel():
                    raise ffi.FusionLibraryError("FusedAdamW.accumulate needs contiguous float32 / bfloat16 gradients of the parameter's size")
                acc = self._acc.get(p)
                if acc is None or acc.shape != p.shape or acc.device != g.device:
                    acc = self._acc[p] = _F._new(p.shape, torch.float32, g.device)      # never zeroed: the first fold overwrites
                    self._acc_fresh.discard(p)
                calls.setdefault((g.dtype, g.device, p not in self._acc_fresh), []).append((p, g, acc))
        for (dtype, device, overwrite), items in calls.items():      # (a parameter whose first gradient of the cycle comes late: its own call)
            n = len(items)
            ffi.check(lib.ff_grad_accumulate(ffi.dtype_code(dtype), n, ffi.ptr_array([g for _, g, _ in items]), ffi.ptr_array([a for _, _, a in items]),
                                             (C.c_longlong * n)(*[g.numel() for _, g, _ in items]), float(scale), int(overwrite),
                                             ffi.stream_handle(device)), "ff_grad_accumulate")
            for p, _, _ in items:
                p.grad = None
                self._acc_fresh.add(p)
        self._acc_open = True

    def accumulated_grad(self, p) -> Optional[torch.Tensor]:
        """The fp32 accumulator of `p` if it was folded into since the last step(), else None."""
        return self._acc[p] if p in self._acc_fresh else None

    def reset_accumulation(self) -> None:
        """Drop an open accumulation cycle without stepping (the accumulators keep their storage; the next accumulate() overwrites)."""
        self._acc_fresh.clear()
        self._acc_open = False

    @torch.no_grad()
    def step(self, closure=None, *, only=None, advance: bool = True, grad_coef: Optional[torch.Tensor] = None):
        """only / advance (capturable mode): update just the parameters whose id() is in `only` - one of several calls that together cover every
        parameter with a gradient exactly once per training step (graphs.PiecewiseGraphedTrainStep(overlap_optimizer=True) updates the
        parameters of a backward segment while the next segments still run).  The FIRST partial call of a training step passes advance=True
        (the device step counters count training steps, not calls) and must execute before the others.  Not with max_grad_norm: the norm
        needs every gradient of the step before the first update.
        grad_coef: a 0-dim fp32 device tensor every gradient is multiplied by - a clip coefficient computed elsewhere (ShardedAdamW's, over
        the gradients of every rank); only without max_grad_norm.
        skip_nonfinite, or `found_inf` / `grad_scale` set by torch.amp.GradScaler.step(): the guarded step (module docstring); neither
        only= (the verdict needs every gradient before the first update) nor grad_coef= (it says nothing about finiteness) goes with it."""
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.step() inside `with swap_ema()`: the parameters hold the averaged weights")
        ext_found, ext_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        amp = ext_found is not None or ext_scale is not None
        guard = self.skip_nonfinite or amp
        if guard and only is not None:
            raise ValueError("FusedAdamW.step(only=...) cannot skip non-finite gradients: the verdict needs every gradient before the first "
                             "update (PiecewiseGraphedTrainStep(overlap_optimizer=True) cannot be used with skip_nonfinite or a GradScaler)")
        if guard and grad_coef is not None:
            raise ValueError("FusedAdamW.step(grad_coef=...) says nothing about the gradients' finiteness: not with skip_nonfinite or a GradScaler")
        if amp:
            if not self._step_supports_amp_scaling:
                raise ValueError("FusedAdamW: found_inf / grad_scale (torch.amp.GradScaler) need capturable=True in every group")
            if self._acc_open:
                raise ValueError("FusedAdamW.step(): found_inf / grad_scale (torch.amp.GradScaler) cannot be combined with an open accumulate() "
                                 "cycle (scaled accumulation is not supported)")
            if ext_found is None and not self.skip_nonfinite:
                raise ValueError("FusedAdamW.step(): grad_scale is set without found_inf")
            for t in (ext_found, ext_scale):
                if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
                    raise ValueError("FusedAdamW.step(): found_inf / grad_scale must be one-element float32 device tensors")
        if self.max_grad_norm is not None and only is not None:
            raise ValueError("FusedAdamW.step(only=...) cannot clip gradients: max_grad_norm needs the norm over every gradient before the first "
                             "update (PiecewiseGraphedTrainStep(overlap_optimizer=True) cannot be used with it)")
        if self.max_grad_norm is not None and grad_coef is not None:
            raise ValueError("FusedAdamW.step(grad_coef=...) replaces the optimizer's own clipping: construct it without max_grad_norm")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        acc = self._acc_open                              # accumulate() was called since the last step: the accumulators are the gradients
        if acc:
            if only is not None:
                raise ValueError("FusedAdamW.step(only=...) cannot be combined with accumulate(): the accumulation cycle is stepped as a whole")
            if any(p.grad is not None for group in self.param_groups for p in group["params"]):
                raise RuntimeError("FusedAdamW.step(): an accumulation cycle is open and a parameter still holds a .grad - the last backward "
                                   "was not folded; call accumulate() after every backward (or reset_accumulation() to drop the cycle)")
        lib = ffi.lib()
        if advance and not torch.cuda.is_current_stream_capturing():
            # an eager training loop cannot run through a timed-out in-launch hand-off of the fused cross-attention kernels unnoticed:
            # looks at the status word the previous step copied to pinned memory, enqueues the next copy; never synchronises
            from . import functional as _F
            _F.poll_sync_exchange("FusedAdamW.step")
        if only is not None:
            only = frozenset(only)
            if not all(g.get("capturable", False) for g in self.param_groups):
                raise ValueError("FusedAdamW.step(only=...) needs capturable=True (step counts live in device scalars shared by the partial calls)")
        if guard:
            coef = self._clip_coef(lib, acc, guard=True, ext_found=ext_found, ext_scale=ext_scale)
        else:
            coef = self._clip_coef(lib, acc) if self.max_grad_norm is not None else grad_coef
        guard = guard and coef is not None                # (no gradient anywhere: nothing to do)
        for gi, group in enumerate(self.param_groups):
            capturable = group.get("capturable", False)
            if capturable and advance:
                # guarded: the counters advance by 1 - skipped, one device add ordered after the guard kernel and before the updates
                self._advance_device_steps(group, self._clip["take"] if guard else None)
            for bucket in self._buckets(gi, group, only, acc):
                params, grad_ptrs, n = bucket["params"], bucket["grad_ptrs"], len(bucket["params"])
                if not acc:
                    self._refresh_grad_ptrs(bucket)
                lr_dev = None
                if capturable:
                    step, step_dev = 0, group["_step_dev"][bucket["device"]].data_ptr()
                    lr_dev = group["_lr_dev"][bucket["device"]].data_ptr()
                else:
                    bucket["step"] += 1                   # the per-parameter `step` entries are refreshed lazily (_sync_host_steps)
                    step, step_dev = bucket["step"], None
                desc = ffi.AdamWDesc(bucket["dtype_code"], n, step, group["lr"], group["betas"][0], group["betas"][1], group["eps"],
                                     group["weight_decay"], group["grad_scale"], step_dev)
                adamw_step_call(lib, desc, bucket["state_code"], (bucket["param_ptrs"], bucket["acc_ptrs"] if acc else grad_ptrs, bucket["m_ptrs"],
                                                                  bucket["v_ptrs"], bucket["w_ptrs"], bucket["numels"]),
                                lr_dev, coef, self._clip["skip"] if guard else None, acc, ffi.stream_handle(bucket["device"]),
                                sr=None if bucket["sr_ids"] is None else (self.sr_seed, bucket["sr_ids"]))
                # the weights were just written: the average follows per bucket, so that the caches get a chance to serve them (host
                # mode knows the step count, so a step that ema_every leaves out issues no launch)
                if self.ema_decay is not None and (capturable or step % self.ema_every == 0):
                    ffi.check(lib.ff_ema_update(bucket["dtype_code"], n, bucket["param_ptrs"], bucket["w_ptrs"], bucket["ema_ptrs"], bucket["numels"],
                                                self.ema_decay, int(self.ema_warmup), self.ema_every, step, step_dev,
                                                self._clip["skip"].data_ptr() if guard else None, ffi.stream_handle(bucket["device"])),
                              "ff_ema_update")
        if acc:
            self.reset_accumulation()                     # the cycle is closed: the next accumulate() overwrites
        return loss

    @staticmethod
    def _refresh_grad_ptrs(bucket) -> None:
        for i, p in enumerate(bucket["params"]):       # only the gradient addresses change from step to step
            g = p.grad
            if g.dtype != p.dtype or not g.is_contiguous():
                raise ffi.FusionLibraryError("FusedAdamW needs contiguous gradients of the parameter's dtype")
            bucket["grad_ptrs"][i] = g.data_ptr()

    def _clip_coef(self, lib, acc: bool = False, guard: bool = False, ext_found=None, ext_scale=None) -> Optional[torch.Tensor]:
        """max_grad_norm: enqueue the global norm of every gradient of every group (grad_scale applied) and the clip coefficient; returns
        the device scalar the AdamW launches of this step read.  No host synchronisation (capturable).  acc: the gradients are the fp32
        accumulators.
        guard: ff_grad_guard instead of ff_grad_clip_coef (the same number of launches), which also writes the verdict; the sweep runs if
        skip_nonfinite or max_grad_norm asks for it, else the verdict is ext_found (a GradScaler's found_inf) alone."""
        buckets = [(group, b) for gi, group in enumerate(self.param_groups) for b in self._buckets(gi, group, None, acc)]
        if not buckets:
            return None
        devices = {b["device"] for _, b in buckets}
        if len(devices) > 1:
            raise ValueError("FusedAdamW(max_grad_norm=...) needs every parameter on one device (the global norm is reduced on it)"
                             if not guard else "FusedAdamW: skipping non-finite gradients needs every parameter on one device")
        device = devices.pop()
        if any(t is not None and t.device != device for t in (ext_found, ext_scale)):
            raise ValueError("FusedAdamW.step(): found_inf / grad_scale must live on the parameters' device")
        sweep = not guard or self.skip_nonfinite or self.max_grad_norm is not None
        clip = self._clip
        if clip is None or clip["device"] != device:
            clip = self._clip = dict(device=device, norm=torch.zeros((), dtype=torch.float32, device=device),
                                     coef=torch.ones((), dtype=torch.float32, device=device),
                                     sum=torch.zeros((), dtype=torch.float64, device=device), partials=None,
                                     skip=None, take=None, total=None, swept=False)
        stream = ffi.stream_handle(device)
        if guard and clip["skip"] is None:
            clip["skip"] = torch.zeros((), dtype=torch.float32, device=device)
            clip["take"] = torch.ones((), dtype=torch.float32, device=device)
            clip["total"] = torch.zeros((), dtype=torch.int64, device=device)
        clip["swept"] = sweep
        if not sweep:
            ffi.check(lib.ff_grad_guard(None, 0.0, ffi.ptr(ext_found), ffi.ptr(ext_scale), None, clip["coef"].data_ptr(), clip["skip"].data_ptr(),
                                        clip["take"].data_ptr(), clip["total"].data_ptr(), stream), "ff_grad_guard")
            return clip["coef"]
        if not acc:
            for _, b in buckets:
                self._refresh_grad_ptrs(b)
        tables = [(ffi.DTYPE_F32 if acc else b["dtype_code"], len(b["params"]), b["acc_ptrs"] if acc else b["grad_ptrs"], b["numels"],
                   float(group["grad_scale"] or 1.0)) for group, b in buckets]
        clip["partials"] = grad_sumsq_sweep(lib, tables, clip["partials"], clip["sum"], False, device, stream)
        if guard:
            ffi.check(lib.ff_grad_guard(clip["sum"].data_ptr(), self.max_grad_norm or 0.0, ffi.ptr(ext_found), ffi.ptr(ext_scale), clip["norm"].data_ptr(),
                                        clip["coef"].data_ptr(), clip["skip"].data_ptr(), clip["take"].data_ptr(), clip["total"].data_ptr(), stream),
                      "ff_grad_guard")
        else:
            ffi.check(lib.ff_grad_clip_coef(clip["sum"].data_ptr(), self.max_grad_norm, clip["norm"].data_ptr(), clip["coef"].data_ptr(), stream),
                      "ff_grad_clip_coef")
        return clip["coef"]

    # ------------------------------------------------------------------ the averaged weights
    def ema_parameters(self):
        """(parameter, its fp32 shadow) for every parameter that has one, in param_groups order (none before the first step)."""
        for group in self.param_groups:
            for p in group["params"]:
                shadow = self.state.get(p, {}).get("ema")
                if shadow is not None:
                    yield p, shadow

    @contextlib.contextmanager
    def swap_ema(self):
        """Evaluate with the averaged weights: inside the block every parameter that has a shadow holds the shadow's value rounded to nearest
        in the parameter's dtype - written IN PLACE, so data_ptr() stays, cached decode sessions are not stale and captured graphs replay on
        the averages.  The weights' own bits wait in a stash of the parameter's dtype and are put back on exit, after an exception too;
        master copies, moments and shadows are not touched.  step(), accumulate() and a nested swap_ema() raise RuntimeError inside the block;
        entering it while a stream is capturing raises as well.  Plain torch copies: this is no hot path."""
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.swap_ema() is not reentrant: the parameters already hold the averaged weights")
        pairs = list(self.ema_parameters())
        if any(p.is_cuda for p, _ in pairs) and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.swap_ema() cannot be entered while a stream is capturing a graph (swap first, then capture or replay)")
        live = [p.detach() for p, _ in pairs]             # (detached views of the same storage: the copies are no autograd operations)
        stash = [t.clone() for t in live]
        self._ema_swapped = True
        try:
            if live:
                torch._foreach_copy_(live, [s for _, s in pairs])
            yield self
        finally:
            if live:
                torch._foreach_copy_(live, stash)
            self._ema_swapped = False

    def sync_device_hyperparams(self) -> None:
        """capturable mode: copy `group["lr"]` into the device scalar the captured kernels read (call before replaying a graph)."""
        for group in self.param_groups:
            for dev, t in group.get("_lr_dev", {}).items():
                if group.get("_lr_on_dev", {}).get(dev) != group["lr"]:
                    t.fill_(float(group["lr"]))
                    group.setdefault("_lr_on_dev", {})[dev] = group["lr"]

    def _buckets(self, gi, group, only=None, acc=False):
        """Parameters with a gradient, grouped by (dtype, device, step count); the pointer tables of everything that does not
        change between steps (parameters, moments, sizes, stochastic-rounding stream ids) are built once and reused while the same parameters have gradients.
        acc: the parameters folded by accumulate() in the open cycle instead, their fp32 accumulators as `acc_ptrs` (the same cache slot,
        so the host-mode step count has one owner whichever kind of step ran last)."""
        if acc:
            active = [p for p in group["params"] if p in self._acc_fresh]
        else:
            active = [p for p in group["params"] if p.grad is not None and (only is None or id(p) in only)]
        cache = self.__dict__.setdefault("_bucket_cache", {})
        key = tuple(id(p) for p in active)
        if acc:
            key = ("acc",) + key
        slot = gi if only is None else (gi, only)
        hit = cache.get(slot)
        if hit is not None and hit[0] == key and all(b["param_ptrs"][0] == b["params"][0].data_ptr() for b in hit[1]) and \
                (not acc or all(b["acc_ptrs"][0] == self._acc[b["params"][0]].data_ptr() for b in hit[1])):
            return hit[1]
        self._sync_host_steps()
        from . import functional as _F
        table = {}
        for p in active:
            ffi.require_cuda(p, self._acc[p] if acc else p.grad)
            if not p.is_contiguous():
                raise ffi.FusionLibraryError("FusedAdamW needs contiguous parameters")
            st = self.state[p]
            mixed = p.dtype == torch.bfloat16          # fp32 parameters are their own master copy and already have fp32 moments
            sdt = self.state_dtype if (mixed and self.state_dtype is not None) else p.dtype
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32)
                st["exp_avg"] = _F._new_zeros_like(p, dtype=sdt)          # (p is contiguous: the same layout preserve_format gives)
                st["exp_avg_sq"] = _F._new_zeros_like(p, dtype=sdt)
            if mixed and self.master_dtype is not None and "master" not in st:
                st["master"] = p.detach().to(torch.float32)
            has_master = "master" in st
            if self.ema_decay is not None and "ema" not in st:      # the weight as it is before its first (or, after a checkpoint without shadows, next) update
                st["ema"] = _F._new_like(p, dtype=torch.float32)
                st["ema"].copy_(st["master"] if has_master else p.detach())
            table.setdefault((p.dtype, p.device, int(st["step"]), st["exp_avg"].dtype, has_master), []).append(p)
        buckets = []
        for (dtype, device, step, sdt, has_master), params in table.items():
            n = len(params)
            buckets.append(dict(params=params, device=device, dtype_code=ffi.dtype_code(dtype), step=step, state_code=ffi.dtype_code(sdt),
                                w_ptrs=ffi.ptr_array([self.state[p]["master"] for p in params]) if has_master else None,
                                param_ptrs=ffi.ptr_array(params), grad_ptrs=(C.c_void_p * n)(),
                                acc_ptrs=ffi.ptr_array([self._acc[p] for p in params]) if acc else None,
                                m_ptrs=ffi.ptr_array([self.state[p]["exp_avg"] for p in params]),
                                v_ptrs=ffi.ptr_array([self.state[p]["exp_avg_sq"] for p in params]),
                                ema_ptrs=ffi.ptr_array([self.state[p]["ema"] for p in params]) if self.ema_decay is not None else None,
                                numels=(C.c_longlong * n)(*[p.numel() for p in params]),
                                # stochastic rounding: the bf16 parameters' stream ids (they have no master copies); None = round to nearest
                                sr_ids=(C.c_uint * n)(*[self._sr_ids[p] for p in params])
                                if self.stochastic_rounding and dtype == torch.bfloat16 and not has_master else None))
        cache[slot] = (key, buckets)
        return buckets

    # ------------------------------------------------------------------ capturable mode
    def _advance_device_steps(self, group, take=None):
        """One float32 step counter per (group, device), advanced by a device-side add (captured along with the update): by 1, or by the
        device scalar `take` (1 - skipped) of a guarded step."""
        counters = group.setdefault("_step_dev", {})
        lrs = group.setdefault("_lr_dev", {})
        for p in group["params"]:
            if (p.grad is not None or p in self._acc_fresh) and p.device not in counters:
                host_steps = [int(self.state[q]["step"]) for q in group["params"] if q in self.state and "step" in self.state[q]]
                counters[p.device] = torch.full((), float(max(host_steps, default=0)), dtype=torch.float32, device=p.device)
                lrs[p.device] = torch.full((), float(group["lr"]), dtype=torch.float32, device=p.device)
                group.setdefault("_lr_on_dev", {})[p.device] = group["lr"]
        if not torch.cuda.is_current_stream_capturing():
            self.sync_device_hyperparams()
        for counter in counters.values():
            counter += 1 if take is None else take

    def _sync_host_steps(self):
        """Write the step counts kept per bucket (host mode) back into the per-parameter state entries."""
        for gi, group in enumerate(self.param_groups):
            if group.get("capturable", False):
                continue
            hit = self.__dict__.get("_bucket_cache", {}).get(gi)
            for bucket in (hit[1] if hit else ()):
                for p in bucket["params"]:
                    self.state[p]["step"] = torch.tensor(float(bucket["step"]), dtype=torch.float32)

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict casts every floating-point state tensor to the PARAMETER's dtype, which would turn the fp32
        moments / master copies of a bf16 parameter into bf16 (and the next step would then either raise or silently continue with bf16
        moments).  The tensors of the incoming state_dict are therefore put back in their own precision afterwards: `master` always in
        fp32, the moments in `state_dtype` (the precision this optimizer was built for) or, without one, the checkpoint's."""
        import copy
        incoming = state_dict["state"]
        saved_groups = state_dict["param_groups"]
        super().load_state_dict(copy.copy(state_dict))
        # map the checkpoint's integer ids to this optimizer's parameters (same order: torch's own rule)
        ids = [i for g in saved_groups for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            src = incoming.get(i)
            st = self.state.get(p)
            if src is None or st is None:
                continue
            mixed = p.dtype == torch.bfloat16
            for key in ("exp_avg", "exp_avg_sq", "master", "ema"):
                if key not in src or not torch.is_tensor(src[key]):
                    continue
                want = torch.float32 if key in ("master", "ema") else (self.state_dtype if (mixed and self.state_dtype is not None) else
                                                              (src[key].dtype if mixed else p.dtype))
                if st[key].dtype != want or st[key].dtype != src[key].dtype:
                    st[key] = src[key].detach().to(device=p.device, dtype=want).clone(memory_format=torch.preserve_format)
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = st["step"].detach().to("cpu", torch.float32)
            if mixed and self.master_dtype is None and "master" in st:
                del st["master"]                       # this optimizer keeps no master copies: the parameter itself is the weight
            if self.ema_decay is None and "ema" in st:
                del st["ema"]                          # ... and this one no average (one that does and finds none starts it at the next step)
        for group in self.param_groups:                # device-side counters of the capturable mode restart from the loaded step counts
            for k in ("_step_dev", "_lr_dev", "_lr_on_dev"):
                group.pop(k, None)
        self.__dict__.pop("_bucket_cache", None)       # moments were replaced: rebuild the pointer tables

    def state_dict(self):
        self._sync_host_steps()
        for group in self.param_groups:      # capturable: bring the host-side `step` entries up to date before serialising
            for device, counter in group.get("_step_dev", {}).items():
                step = float(counter)
                for p in group["params"]:
                    if p in self.state and p.device == device:
                        self.state[p]["step"] = torch.tensor(step, dtype=torch.float32)
        out = super().state_dict()
        for g in out["param_groups"]:
            for k in ("_step_dev", "_lr_dev", "_lr_on_dev"):
                g.pop(k, None)
        return out


def adamw_step_call(lib, desc, state_code, ptrs, lr_dev, coef, skip, grads_fp32, stream, sr=None) -> None:
    """The one call site of the AdamW entry points.  ptrs: the pointer tables (params, grads, exp_avg, exp_avg_sq, master or None, numels);
    coef / skip: the 0-dim device tensors of the clip coefficient and of the guard's verdict, or None; grads_fp32: the gradients are the
    fp32 accumulators of ff_grad_accumulate.  skip -> ff_adamw_step_guarded, else grads_fp32 -> ff_adamw_step_acc (coef optional), else
    coef -> ff_adamw_step_clipped, else ff_adamw_step_mixed.  sr: (seed, stream ids as a C unsigned array, one per tensor) ->
    ff_adamw_step_sr, which takes coef, skip and grads_fp32 as they are (bf16 parameters without master copies)."""
    p, g, m, v, w, numels = ptrs
    c = None if coef is None else coef.data_ptr()
    if sr is not None:
        if w is not None:
            raise ffi.FusionLibraryError("stochastic rounding is for parameters without fp32 master copies")
        seed, ids = sr
        ffi.check(lib.ff_adamw_step_sr(desc, state_code, p, g, int(grads_fp32), m, v, lr_dev, c, None if skip is None else skip.data_ptr(),
                                       seed - (seed >> 63 << 64), ids, numels, stream), "ff_adamw_step_sr")
        return
    if skip is not None:
        name, args = "ff_adamw_step_guarded", (p, g, int(grads_fp32), m, v, w, lr_dev, c, skip.data_ptr())
    elif grads_fp32:
        name, args = "ff_adamw_step_acc", (p, g, m, v, w, lr_dev, c)
    elif coef is None:
        name, args = "ff_adamw_step_mixed", (p, g, m, v, w, lr_dev)
    else:
        name, args = "ff_adamw_step_clipped", (p, g, m, v, w, lr_dev, c)
    ffi.check(getattr(lib, name)(desc, state_code, *args, numels, stream), name)


def grad_tables(grads, who: str) -> list:
    """Contiguous fp32 / bf16 gradient tensors as one (dtype code, n, pointer table, numels, scale 1.0) per dtype: what grad_sumsq_sweep
    and ff_scale_grads take."""
    tables = []
    for dt in (torch.float32, torch.bfloat16):
        gs = [g for g in grads if g.dtype == dt]
        if gs:
            if not all(g.is_contiguous() for g in gs):
                raise ffi.FusionLibraryError(f"{who} needs contiguous gradients")
            tables.append((ffi.dtype_code(dt), len(gs), ffi.ptr_array(gs), (C.c_longlong * len(gs))(*[g.numel() for g in gs]), 1.0))
    if sum(t[1] for t in tables) != len(grads):
        raise ffi.FusionLibraryError(f"{who} handles float32 and bfloat16 gradients")
    return tables


def grad_sumsq_sweep(lib, tables, partials, total, accumulate: bool, device, stream):
    """The sum-of-squares sweep: *total = (accumulate ? *total : 0) + the sum of (scale * g)^2 over every tensor of `tables` [(dtype code, n,
    pointer table, numels, scale)] - one ff_grad_sumsq per table, their per-workgroup slots continuing from table to table, and one
    ff_grad_sumsq_reduce (fp64).  partials: the caller's slot buffer from an earlier sweep or None; returns the buffer used (a new one
    where that was too small - every slot that is read is written first, so it is not zeroed).  Enqueues only."""
    slots = [int(lib.ff_grad_sumsq_partials(n, numels)) for _, n, _, numels, _ in tables]
    if partials is None or partials.numel() < sum(slots):
        partials = torch.empty(max(sum(slots), 1), dtype=torch.float32, device=device)
    off = 0
    for (code, n, ptrs, numels, scale), k in zip(tables, slots):      # slots continue from table to table (dtypes, groups)
        ffi.check(lib.ff_grad_sumsq(code, n, ptrs, numels, scale, partials.data_ptr() + 4 * off, partials.numel() - off, stream), "ff_grad_sumsq")
        off += k
    ffi.check(lib.ff_grad_sumsq_reduce(partials.data_ptr(), off, total.data_ptr(), int(accumulate), stream), "ff_grad_sumsq_reduce")
    return partials


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (norm_type 2) on the device: the total L2 norm of the gradients of `parameters` (fp32 0-dim tensor,
    summed in fp32 per workgroup and in fp64 over workgroups, also for bf16 gradients) is returned, and every gradient is multiplied in
    place by min(1, max_norm / (norm + 1e-6)).  A non-finite norm propagates as in torch; error_if_nonfinite=True raises instead (one host
    synchronisation, as in torch).  Gradients: contiguous fp32 / bf16 on one device."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ computes the L2 norm only (norm_type=2), got norm_type={norm_type}")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    devices = {g.device for g in grads}
    if len(devices) > 1:
        raise ValueError("clip_grad_norm_ needs every gradient on one device")
    ffi.require_cuda(*grads)
    device = devices.pop()
    lib = ffi.lib()
    stream = ffi.stream_handle(device)
    tables = grad_tables(grads, "clip_grad_norm_")
    total = torch.empty((), dtype=torch.float64, device=device)
    norm = torch.empty((), dtype=torch.float32, device=device)
    coef = torch.empty((), dtype=torch.float32, device=device)
    grad_sumsq_sweep(lib, tables, None, total, False, device, stream)
    ffi.check(lib.ff_grad_clip_coef(total.data_ptr(), float(max_norm), norm.data_ptr(), coef.data_ptr(), stream), "ff_grad_clip_coef")
    if error_if_nonfinite and not bool(torch.isfinite(norm)):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    for code, n, ptrs, numels, _ in tables:
        ffi.check(lib.ff_scale_grads(code, n, ptrs, numels, coef.data_ptr(), stream), "ff_scale_grads")
    return norm
