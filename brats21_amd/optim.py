"""Ranger2020 with the reference's constructor and state layout (learning/optimizer.py:62-135), stepped by
two HIP launches over all parameters (csrc/ranger.hip) instead of the reference's per-tensor Python loop of
~15 small torch ops each (:145-253).

``state_dict()`` / ``load_state_dict()`` are the reference's: per parameter ``step``, ``exp_avg``,
``exp_avg_sq``, ``slow_buffer`` -- so Engine.resume (learning/engine.py:511-525) restores either way.

``clip_grad_norm_`` (torch.nn.utils.clip_grad_norm_, the reference's --gradient_clipping) and ``AGC`` (the reference's
learning/lr_scheduler.py:133-241, its --adaptive_gradient_clipping) run on the same kind of device table in at most three
launches over all gradients (csrc/gradclip.hip), without a host round trip, so both capture into the step's hipGraph.
"""
import math
import os
from collections.abc import Iterable

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import _lib

_REC = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("slow", "<u8"),
                 ("numel", "<i8"), ("rowlen", "<i4"), ("row_base", "<i4"), ("neg_step", "<f4"), ("wd", "<f4"),
                 ("flags", "<i4"), ("chunk_base", "<i4")])  # == brats_ranger_tensor (include/brats_hip.h)


_CLIP_REC = np.dtype([("param", "<u8"), ("grad", "<u8"), ("numel", "<i8"), ("unit_len", "<i4"), ("unit_stride", "<i4"),
                      ("unit_base", "<i4"), ("nunits", "<i4")])  # == brats_gradclip_tensor (include/brats_hip.h)


class _DeviceTable:
    """Per-tensor records on the host (a numpy record array, rewritten per step: gradient pointers, step scalars) and their
    copy on the device.  The copy is asynchronous from a ring of pinned staging buffers -- a slot is reused only after its
    copy ran -- and, while a stream is capturing, from one fixed pinned buffer: the graph's memcpy node re-reads that buffer
    at every replay, so nobody may rewrite it afterwards (it is allocated here because pinning memory is not allowed during
    a capture)."""

    def __init__(self, rec, dev):
        self.rec = rec
        self.pinned = [torch.empty(rec.nbytes, dtype=torch.uint8).pin_memory() for _ in range(4)]
        self.pinned_capture = torch.empty(rec.nbytes, dtype=torch.uint8).pin_memory()
        self.events = [None] * 4
        self.dev = torch.empty(rec.nbytes, dtype=torch.uint8, device=dev)
        self.slot = 0

    def upload(self, capturing):
        """Copy the host records to the device table on the current stream; returns the device table."""
        if capturing:
            pinned = self.pinned_capture
            pinned.numpy()[:] = self.rec.view(np.uint8)
            self.dev.copy_(pinned, non_blocking=True)
        else:
            slot = self.slot
            self.slot = (slot + 1) % 4
            if self.events[slot] is not None:
                self.events[slot].synchronize()
            pinned = self.pinned[slot]
            pinned.numpy()[:] = self.rec.view(np.uint8)
            self.dev.copy_(pinned, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.events[slot] = ev
        return self.dev


def radam_step_size(step, beta1, beta2, n_sma_threshold):
    """learning/optimizer.py:198-214 -> (N_sma > threshold, step_size)."""
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > n_sma_threshold:
        return True, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (
            1 - beta1 ** step)
    return False, 1.0 / (1 - beta1 ** step)


class Ranger2020(Optimizer):
    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, use_gcnorm=False, normloss=False, normloss_factor=1e-4, gc_conv_only=False, gc_loc=True,
                 capturable=False):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not lr > 0:
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        if normloss:
            # learning/optimizer.py:192-198: p.mul_() on a leaf that requires grad, outside torch.no_grad() -- the reference's
            # own step() raises RuntimeError there, so there is no behaviour to reproduce
            raise NotImplementedError("Ranger2020(normloss=True) is not built: the reference's step() itself fails on it "
                                      "(in-place operation on a leaf Variable, learning/optimizer.py:198)")
        if not gc_loc:
            raise NotImplementedError("brats21_amd.optim.Ranger2020 implements gc_loc=True (the reference's default)")
        defaults = dict(lr=lr, alpha=alpha, k=k, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold, self.alpha, self.k = N_sma_threshhold, alpha, k
        self.use_gc, self.gc_conv_only, self.eps = use_gc, gc_conv_only, eps
        self.use_gcnorm = use_gcnorm
        # capturable (extension, like torch.optim.Adam's): the step counter and the RAdam scalars live on the device,
        # so a step captured into a hipGraph (engine.GraphedTrainStep) replays without host-side changes.  All
        # parameters of a group then share one step count; the learning rate is a device scalar too (sync_lr() rewrites
        # it when an LR scheduler changed group["lr"]: no re-capture).
        self.capturable = capturable
        self._plans = {}
        # torch.amp.GradScaler protocol (as torch's fused Adam): GradScaler.step() then hands the loss scale and the overflow flag
        # over as DEVICE tensors (self.grad_scale / self.found_inf) instead of reading the flag on the host and unscaling in a
        # pass of its own.  capturable=True: the skip is decided on the device too (no host round trip per step); otherwise the
        # flag is read here -- the reference loop's own synchronisation (learning/engine.py:117-122), no more
        self._step_supports_amp_scaling = os.environ.get("BRATS_RANGER_AMP", "1") != "0"  # (0: GradScaler's own unscale pass + host check, for A/B runs)

    # ------------------------------------------------------------------------------------------ static plan
    def _plan(self, gi, active, dev):
        """chunk / row tables for the set of parameters that have a gradient (static per model)."""
        key = (gi, tuple(id(p) for p in active))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        chunk = _lib.lib().brats_ranger_chunk()
        chunks, rows, rowlen, rowbase, nrows, chunkbase, nch = [], [], [], [], 0, [], 0
        for t, p in enumerate(active):
            n = p.numel()
            chunkbase.append(nch)
            nch += (n + chunk - 1) // chunk
            chunks.append(np.stack([np.full((n + chunk - 1) // chunk, t, np.int32),
                                    np.arange((n + chunk - 1) // chunk, dtype=np.int32)], 1))
            gc = self.use_gc and p.dim() > (3 if self.gc_conv_only else 1)
            if gc:
                r = p.shape[0]
                rows.append(np.stack([np.full(r, t, np.int32), np.arange(r, dtype=np.int32)], 1))
                rowlen.append(n // r)
                rowbase.append(nrows)
                nrows += r
            else:
                rowlen.append(0)
                rowbase.append(0)
        plan = {
            "chunks": torch.from_numpy(np.concatenate(chunks)).to(dev),
            "rows": torch.from_numpy(np.concatenate(rows)).to(dev) if rows else None,
            "means": torch.empty(max(nrows, 1), dtype=torch.float32, device=dev),
            "nrows": nrows, "rowlen": rowlen, "rowbase": rowbase, "chunkbase": chunkbase,
            # use_gcnorm workspaces: per-chunk (sum, sum of squares) and the per-tensor standard deviation
            "chunk_stats": torch.empty((nch, 2), dtype=torch.float32, device=dev) if self.use_gcnorm else None,
            "grad_std": torch.empty(len(active), dtype=torch.float32, device=dev) if self.use_gcnorm else None,
        }
        self._plans[key] = plan
        return plan

    # ------------------------------------------------------------------------------------------ step
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}  # the state tensors were replaced: cached pointer tables are stale

    def sync_lr(self):
        """capturable mode: copy every group's current lr into its device scalar (call between graph replays after an LR
        scheduler stepped; GraphedTrainStep does).  A no-op while nothing changed."""
        for (gi, _), plan in self._plans.items():
            dyn = plan.get("dyn")
            if dyn is not None:
                lr = float(self.param_groups[gi]["lr"])
                if plan.get("lr_dev") != lr:
                    if torch.cuda.is_current_stream_capturing():
                        raise _lib.BratsHipError("Ranger2020: the learning rate changed inside a hipGraph capture")
                    dyn[4:6].view(torch.float64).fill_(lr)
                    plan["lr_dev"] = lr

    def sync_steps(self):
        """capturable mode: graph replays advance only the device-side step counters; copy them into state['step']."""
        for plan in self._plans.values():
            if plan.get("dyn") is not None:
                step = int(plan["dyn"][0].item())
                for st in plan["states"]:
                    st['step'] = step

    def state_dict(self):
        self.sync_steps()
        return super().state_dict()

    def _table(self, plan, active, dev):
        """Host copy of the per-tensor records.  Parameter / state pointers and shapes never change between steps
        (cached); per step only the gradient pointers and the step-dependent scalars are rewritten -- the reference's
        Python loop over parameters (learning/optimizer.py:145-253) must not come back as host time here."""
        rec = plan.get("rec")
        if rec is not None:
            # the cached records hold raw addresses: parameters or state tensors re-allocated since (model.to() / .half()
            # / .float() round trips, load_state_dict(assign=True), p.data = ..., a state replaced by hand) must not be
            # written through the old ones
            ptrs = plan["ptrs"]
            for t, p in enumerate(active):
                st = self.state[p]
                if (p.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['slow_buffer'].data_ptr()) != ptrs[t]:
                    rec = None
                    break
        if rec is None:
            rec = np.zeros(len(active), _REC)
            for t, p in enumerate(active):
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                    raise _lib.BratsHipError("Ranger2020: parameters must be contiguous f32 tensors on one GPU")
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['slow_buffer'] = p.detach().clone(memory_format=torch.contiguous_format)
                else:
                    for name in ('exp_avg', 'exp_avg_sq', 'slow_buffer'):  # after load_state_dict / .cpu() round trips
                        s = state[name]
                        if s.dtype != torch.float32 or s.device != dev or not s.is_contiguous():
                            state[name] = s.to(device=dev, dtype=torch.float32).contiguous()
                    state['step'] = int(state['step'])
                rec[t] = (p.data_ptr(), 0, state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(),
                          state['slow_buffer'].data_ptr(), p.numel(), plan["rowlen"][t], plan["rowbase"][t], 0.0, 0.0, 0, plan["chunkbase"][t])
            plan["rec"] = rec
            plan["states"] = [self.state[p] for p in active]
            plan["ptrs"] = [(int(r["param"]), int(r["exp_avg"]), int(r["exp_avg_sq"]), int(r["slow"])) for r in rec]
            plan["table"] = _DeviceTable(rec, dev)
        return rec

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.lib()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        if found_inf is not None and not self.capturable:
            if float(found_inf.item()) != 0.0:  # GradScaler's skipped step: nothing moves, the step counts stay
                return None
            found_inf = None
        for t_ in (grad_scale, found_inf):
            if t_ is not None and (t_.dtype != torch.float32 or t_.numel() != 1 or not t_.is_cuda):
                raise _lib.BratsHipError("Ranger2020: grad_scale / found_inf must be one-element f32 device tensors (torch.amp.GradScaler's)")
        for gi, group in enumerate(self.param_groups):
            active = [p for p in group["params"] if p.grad is not None]
            if not active:
                continue
            dev = active[0].device
            if dev.type != "cuda":
                raise _lib.BratsHipError("brats21_amd.optim.Ranger2020 steps on the GPU only (no CPU fallback)")
            beta1, beta2 = group["betas"]
            lr, wd, k = group["lr"], group["weight_decay"], group["k"]
            plan = self._plan(gi, active, dev)
            if self.capturable and plan.get("dyn") is None and not torch.cuda.is_current_stream_capturing():
                # a plan about to get its device-side step counter: the host-side state['step'] runs AHEAD of the device after
                # overflow-skipped steps (the skip is decided on the device) -- seed it from the device's truth
                self.sync_steps()
            rec = self._table(plan, active, dev)
            keep = []
            grads = rec["grad"]
            for t, p in enumerate(active):
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                    if g.is_sparse:
                        raise RuntimeError('Ranger optimizer does not support sparse gradients')
                    g = g.float().contiguous()
                    keep.append(g)
                grads[t] = g.data_ptr()
            states = plan["states"]
            steps = [st['step'] + 1 for st in states]
            for st, v in zip(states, steps):
                st['step'] = v
            cache = {}
            neg, flags = rec["neg_step"], rec["flags"]
            for t, v in enumerate(steps):
                c = cache.get(v)
                if c is None:
                    adaptive, step_size = radam_step_size(v, beta1, beta2, self.N_sma_threshhold)
                    c = cache[v] = (-step_size * lr, (1 if adaptive else 0) | (2 if v % k == 0 else 0))
                neg[t], flags[t] = c
            rec["wd"] = wd
            capturing = torch.cuda.is_current_stream_capturing()
            stream = torch.cuda.current_stream().cuda_stream
            dyn = None
            if self.capturable:
                if len(cache) != 1:
                    raise _lib.BratsHipError("Ranger2020(capturable=True): all parameters of a group must share one step count")
                dyn = plan.get("dyn")
                if dyn is None:  # brats_ranger_dyn {step, flags, neg_step, reserved, double lr}; step = the count BEFORE this step
                    if capturing:
                        raise _lib.BratsHipError("Ranger2020(capturable=True): run one eager step before capturing (state allocation)")
                    dyn = plan["dyn"] = torch.tensor([steps[0] - 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
                if not capturing:
                    self.sync_lr()
                elif plan.get("lr_dev") != float(lr):
                    raise _lib.BratsHipError("Ranger2020: the learning rate changed between the warm-up steps and the capture")
                _lib.check(lib.brats_ranger_advance_amp(dyn.data_ptr(), -1.0, float(beta1), float(beta2), int(k),
                                                        float(self.N_sma_threshhold),
                                                        found_inf.data_ptr() if found_inf is not None else None, stream), "ranger_advance")
            elif capturing:
                raise _lib.BratsHipError("Ranger2020.step() inside a hipGraph capture needs capturable=True")
            table = plan["table"].upload(capturing)
            _lib.check(lib.brats_ranger_step_amp(
                table.data_ptr(), len(active), plan["chunks"].data_ptr(), plan["chunks"].shape[0],
                plan["rows"].data_ptr() if plan["rows"] is not None else None, plan["nrows"], plan["means"].data_ptr(),
                plan["chunk_stats"].data_ptr() if self.use_gcnorm else None, plan["grad_std"].data_ptr() if self.use_gcnorm else None,
                dyn.data_ptr() if dyn is not None else None, beta1, beta2, 1 - beta1, 1 - beta2, group["eps"], self.alpha,
                grad_scale.data_ptr() if grad_scale is not None else None, found_inf.data_ptr() if found_inf is not None else None,
                stream), "ranger_step")
            for p in active:  # the kernel wrote through raw pointers: tell autograd / the packed-weight cache
                torch.autograd.graph.increment_version(p)
        return None


# ---------------------------------------------------------------------------------------------- gradient clipping
def unit_layout(shape, agc=True):
    """(nunits, unit_len, unit_stride) of the reference's ``unitwise_norm`` (learning/lr_scheduler.py:114-130): the whole tensor
    for ndim <= 1, one unit per trailing index (norm over dim 0: strided columns) for ndim 2 / 3, one unit per slice along dim 0
    for ndim 4 / 5.  Other ranks: ValueError as in the reference; for global-norm clipping alone (agc=False), where the units
    are only a decomposition of the sum, they are cut along dim 0 as well."""
    numel = 1
    for d in shape:
        numel *= int(d)
    if len(shape) <= 1:
        return 1, numel, 1
    rows = int(shape[0])
    if len(shape) in (2, 3):
        return numel // rows, rows, numel // rows
    if len(shape) in (4, 5) or not agc:
        return rows, numel // rows, 1
    raise ValueError('Wrong input dimensions')


class _ClipPlan:
    """Static tables of one set of tensors (units, chunks, the stats workspace) + the per-step record table."""

    def __init__(self, params, dev, agc):
        lib = _lib.lib()
        chunk = lib.brats_gradclip_chunk()
        self.params = params  # (kept alive: the cache key is their ids)
        self.shapes = [p.shape for p in params]
        rec = np.zeros(len(params), _CLIP_REC)
        units, chunks, nunits = [], [], 0
        for t, p in enumerate(params):
            n = p.numel()
            if n >= 2 ** 31:
                raise _lib.BratsHipError("gradient clipping: a tensor has 2^31 or more elements")
            nu, ulen, ustride = unit_layout(p.shape, agc)
            rec[t] = (0, 0, n, ulen, ustride, nunits, nu)
            units.append(np.stack([np.full(nu, t, np.int32), np.arange(nu, dtype=np.int32)], 1))
            nch = (n + chunk - 1) // chunk
            chunks.append(np.stack([np.full(nch, t, np.int32), np.arange(nch, dtype=np.int32)], 1))
            nunits += nu
        self.units = torch.from_numpy(np.concatenate(units)).to(dev)
        self.chunks = torch.from_numpy(np.concatenate(chunks)).to(dev)
        self.stats = torch.zeros((nunits, 2), dtype=torch.float32, device=dev)
        self.table = _DeviceTable(rec, dev)

    def run(self, what, max_norm, clipping, eps, grad_scale, found_inf):
        """One brats_gradclip call on the current gradients.  max_norm None: no global norm; clipping None: no AGC.  Returns
        the {total_norm, clip_coef} device pair, or None."""
        rec, dev = self.table.rec, self.stats.device
        pptr, gptr = rec["param"], rec["grad"]
        for t, p in enumerate(self.params):
            g = p.grad
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev or g.shape != p.shape:
                raise _lib.BratsHipError(f"{what}: gradients must be contiguous f32 tensors on the parameters' GPU (the pass works "
                                         "in place: it cannot run on a converted copy)")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.BratsHipError(f"{what}: parameters must be contiguous f32 tensors")
            pptr[t], gptr[t] = p.data_ptr(), g.data_ptr()
        for t_ in (grad_scale, found_inf):
            if t_ is not None and (t_.dtype != torch.float32 or t_.numel() != 1 or t_.device != dev):
                raise _lib.BratsHipError(f"{what}: grad_scale / found_inf must be one-element f32 device tensors (torch.amp.GradScaler's)")
        table = self.table.upload(torch.cuda.is_current_stream_capturing())
        # (a fresh pair per call: the returned total norm is not overwritten by the next call; no launch, under capture it
        # comes from the graph's pool)
        pair = torch.empty(2, dtype=torch.float32, device=dev) if max_norm is not None else None
        _lib.check(_lib.lib().brats_gradclip(
            table.data_ptr(), len(self.params), self.units.data_ptr(), self.units.shape[0], self.chunks.data_ptr(),
            self.chunks.shape[0], self.stats.data_ptr(), pair.data_ptr() if pair is not None else None,
            float(max_norm) if max_norm is not None else -1.0, float(clipping) if clipping is not None else -1.0, float(eps),
            grad_scale.data_ptr() if grad_scale is not None else None, found_inf.data_ptr() if found_inf is not None else None,
            torch.cuda.current_stream().cuda_stream), what)
        return pair


_CLIP_PLANS = {}  # clip_grad_norm_'s plans, newest last (AGC keeps its own)


def _clip(plans, what, params, max_norm, clipping, eps, grad_scale, found_inf, limit=8):
    active = [p for p in params if p.grad is not None and p.numel() > 0]
    if not active:
        return None
    dev = active[0].device
    if dev.type != "cuda" or any(p.device != dev for p in active):
        raise _lib.BratsHipError(f"brats21_amd.optim.{what} runs on one GPU only (no CPU fallback)")
    key = (clipping is not None,) + tuple(id(p) for p in active)
    plan = plans.get(key)
    if plan is None or any(a.shape != b for a, b in zip(active, plan.shapes)):
        plan = plans[key] = _ClipPlan(active, dev, clipping is not None)
        while len(plans) > limit:
            del plans[next(iter(plans))]
    return plan.run(what, max_norm, clipping, eps, grad_scale, found_inf)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, grad_scale=None,
                    found_inf=None):
    """torch.nn.utils.clip_grad_norm_ in three launches over all gradients (csrc/gradclip.hip): the 2-norm over every gradient,
    ``clip_coef = min(1, max_norm / (total_norm + 1e-6))``, gradients scaled in place.  Returns the total norm as a 0-dim f32
    device tensor; nothing touches the host.  ``foreach`` is accepted and ignored.

    grad_scale / found_inf (extension, the GradScaler pair of Ranger2020): one-element f32 device tensors.  With grad_scale the
    gradients still carry that loss scale: the norm is the unscaled gradients', the gradients stay scaled.  With found_inf
    non-zero nothing is written (the returned norm is then undefined)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise NotImplementedError("brats21_amd.optim.clip_grad_norm_ implements norm_type=2 (the reference's)")
    if error_if_nonfinite:
        raise NotImplementedError("brats21_amd.optim.clip_grad_norm_: error_if_nonfinite=True would read the norm on the host")
    max_norm = float(max_norm)
    if max_norm < 0:
        raise ValueError(f"Invalid max_norm: {max_norm}")
    parameters = list(parameters)
    pair = _clip(_CLIP_PLANS, "clip_grad_norm_", parameters, max_norm, None, 0.0, grad_scale, found_inf)
    if pair is None:  # no gradients at all: torch returns 0.
        return torch.zeros((), dtype=torch.float32, device=parameters[0].device if parameters else None)
    return pair[0]


@torch.no_grad()
def clip_grad_norm_agc_(parameters, max_norm, clipping=1e-2, eps=1e-3, *, grad_scale=None, found_inf=None):
    """``clip_grad_norm_(parameters, max_norm)`` followed by the clipping pass of ``AGC(parameters, ..., clipping, eps)`` -- the
    reference's order -- as ONE call of three launches: the per-unit sums are taken once and AGC's unit norms are those of the
    globally clipped gradient, ``clip_coef * ||g_unit||``.  Returns the total norm (before clipping) like clip_grad_norm_."""
    max_norm = float(max_norm)
    if max_norm < 0 or clipping < 0 or eps < 0:
        raise ValueError(f"Invalid max_norm / clipping / eps: {max_norm}, {clipping}, {eps}")
    parameters = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    pair = _clip(_CLIP_PLANS, "clip_grad_norm_agc_", parameters, max_norm, clipping, eps, grad_scale, found_inf)
    if pair is None:
        return torch.zeros((), dtype=torch.float32, device=parameters[0].device if parameters else None)
    return pair[0]


class AGC(Optimizer):
    """Adaptive gradient clipping around any optimizer: the reference's ``AGC`` (learning/lr_scheduler.py:133-241) with its
    constructor, its errors and its shared ``param_groups`` / ``state``; ``step()`` clips every unit of every gradient (a unit is
    what ``unitwise_norm`` takes a norm over) to ``clipping * max(||p_unit||, eps)`` in two launches over all tensors instead of a
    dozen torch ops and two host-to-device uploads per tensor, then steps the wrapped optimizer.

    Two departures from the reference:
      1. ``params`` is materialised with ``list()``.  The reference keeps what it is given, and its only call site passes
         ``model.parameters()``, a generator: its first ``step()`` exhausts it and from the second step on nothing is clipped.
         This class clips at every step.
      2. With ``model=``, every parameter is taken once.  The reference collects ``module.parameters()`` of every module that is
         not named in ``ignore_agc`` -- the root module included, so a parameter appears once per enclosing module and is clipped
         that many times (the repeats change nothing but rounding), and the ignored modules' parameters come in through their
         parents all the same.  The set of parameters is the reference's.

    torch.amp.GradScaler: the wrapper declares ``_step_supports_amp_scaling`` (and ``capturable``) exactly when the wrapped
    optimizer does; the loss scale and the overflow flag that GradScaler.step() then leaves on the wrapper are used by the AGC
    kernels (norms of the unscaled gradient; no-op on overflow) and handed to the wrapped optimizer while it steps."""

    def __init__(self, params, optim, clipping=1e-2, eps=1e-3, model=None, ignore_agc=("fc",)):
        if clipping < 0.0:
            raise ValueError("Invalid clipping value: {}".format(clipping))
        if eps < 0.0:
            raise ValueError("Invalid eps value: {}".format(eps))
        self.optim = optim
        if not isinstance(ignore_agc, Iterable):
            ignore_agc = [ignore_agc]
        if model is not None:
            assert ignore_agc not in [None, []], "You must specify ignore_agc for AGC to ignore fc-like(or other) layers"
            names = [name for name, module in model.named_modules()]
            for module_name in ignore_agc:
                if module_name not in names:
                    raise ModuleNotFoundError("Module name {} not found in the model".format(module_name))
            seen, plist = set(), []
            for name, module in model.named_modules():
                if name not in ignore_agc:
                    for p in module.parameters():
                        if id(p) not in seen:
                            seen.add(id(p))
                            plist.append(p)
        else:
            plist = []
            for p in params:  # tensors, or the parameter-group dicts torch's optimizers accept
                plist.extend(p["params"] if isinstance(p, dict) else [p])
        for p in plist:
            unit_layout(p.shape)  # (a rank unitwise_norm does not know raises here, not at the first step)
        self.agc_params = [{"params": plist}]
        self.eps = eps
        self.clipping = clipping
        self._clip_plans = {}

    # the wrapped optimizer's, not copies: load_state_dict() replaces both objects
    @property
    def param_groups(self):
        return self.optim.param_groups

    @property
    def state(self):
        return self.optim.state

    @property
    def defaults(self):
        return {"clipping": self.clipping, "eps": self.eps, **self.optim.defaults}

    @property
    def _step_supports_amp_scaling(self):
        return getattr(self.optim, "_step_supports_amp_scaling", False)

    @property
    def capturable(self):
        return getattr(self.optim, "capturable", False) or all(g.get("capturable", False) for g in self.optim.param_groups)

    def __getattr__(self, name):
        if name in ("sync_lr", "sync_steps"):  # engine.GraphedTrainStep refreshes the device-side learning rate through these
            return getattr(self.__dict__["optim"], name)
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    @torch.no_grad()
    def clip_(self, grad_scale=None, found_inf=None):
        """The clipping pass alone (two launches), in place on the gradients; step() runs it before the wrapped step."""
        _clip(self._clip_plans, "AGC", self.agc_params[0]["params"], None, self.clipping, self.eps, grad_scale, found_inf, limit=2)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            with torch.enable_grad():
                closure()
        # what GradScaler.step() put on this object (instance attributes, removed by it afterwards)
        grad_scale, found_inf = self.__dict__.get("grad_scale"), self.__dict__.get("found_inf")
        self.clip_(grad_scale, found_inf)
        if grad_scale is None and found_inf is None:
            return self.optim.step(closure)
        self.optim.grad_scale, self.optim.found_inf = grad_scale, found_inf
        try:
            return self.optim.step(closure)
        finally:
            del self.optim.grad_scale, self.optim.found_inf

    def zero_grad(self, set_to_none=False):
        return self.optim.zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        return self.optim.state_dict()

    def load_state_dict(self, state_dict):
        return self.optim.load_state_dict(state_dict)
