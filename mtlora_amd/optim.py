"""The parameter update of the train step on the HIP path (csrc/optim.hip): gradient norm, clip, loss-scale unscale, inf / nan
skip, AdamW and the scaler update as THREE launches for all trainable tensors, with no host synchronisation.

Replaces the reference's ``NativeScalerWithGradNormCount`` + ``torch.optim.AdamW`` pair (utils.py:348-375, optimizer.py:71-85,
called at main.py:347-353):

    optimizer = FusedAdamW(param_groups, lr=..., weight_decay=...)
    loss_scaler = LossScaler()
    grad_norm = loss_scaler(loss, optimizer, clip_grad=5.0, update_grad=(idx + 1) % accumulation_steps == 0)

``FusedSGD`` (momentum, Nesterov: three launches) and ``FusedLAMB`` (apex's algorithm: four launches) are the reference's other
two optimizers (optimizer.py:53-66) on the same machinery, which the base class ``FusedOptimizer`` carries; ``sgd_update_torch`` and
``lamb_update_torch`` state in plain torch what their kernels compute.

fp32 parameters, gradients and state only; there is no fallback: anything else raises.
"""
from __future__ import annotations

import ctypes
import math
from typing import Any, Dict, List, Optional

import torch

from . import _lib

__all__ = ["FusedOptimizer", "FusedAdamW", "FusedSGD", "FusedLAMB", "LossScaler", "uniform_step", "accumulation_steps_of",
           "sgd_update_torch", "lamb_update_torch"]

_STATE_ALIGN = 4  # elements: every tensor's slice of the flat state buffers starts 16-byte aligned
_HYPER_SLOTS = 4  # pinned staging slots of a capturable optimizer's hyper-parameter uploads
_GROUP_WORDS = 5  # doubles per mtlora_adamw_group record


def uniform_step(state: Dict[Any, Dict[str, Any]], who: str = "FusedAdamW") -> float:
    """the one step count of an AdamW ``state`` mapping (``state_dict()["state"]`` or ``optimizer.state``); 0 if it is empty.
    The kernels keep ONE device counter for all parameters, so a state whose per-parameter steps differ cannot be represented."""
    steps = {float(s["step"]) for s in state.values() if "step" in s}
    if len(steps) > 1:
        raise ValueError(f"mtlora_amd: {who} keeps one step counter for all parameters; this state has steps {sorted(steps)}")
    return steps.pop() if steps else 0.0


def accumulation_steps_of(k: Any) -> int:
    """``k`` as a gradient-accumulation step count (the reference's ``TRAIN.ACCUMULATION_STEPS``): an integer >= 1, else ValueError"""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.ADAMW_MAX_ACCUM_STEPS:
        raise ValueError(f"mtlora_amd: accumulation_steps must be an integer in [1, {_lib.ADAMW_MAX_ACCUM_STEPS}], got {k!r}")
    return k


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers of this module share (``FusedAdamW``, ``FusedSGD``, ``FusedLAMB``; ``mtl_harness`` and
    ``checkpoint`` test for this class): the construction checks, the tensor / chunk table and the flat state buffers, the staging
    of the gradient pointers, ``clip_and_step(max_norm, scaler)`` -- norm, clip, unscale, inf / nan skip and scaler update on the
    device -- and ``step()``, the capturable form (``push_hyperparameters()``, ``bump_versions()``, ``reset_capture()``) and the
    snapshot interface (``state_tensors()`` / ``state_meta()`` / ``state_dict_from()``).  A subclass names its state entries
    (``_STATE_KEYS``: what the one or two flat buffers are called in ``state[p]``), says whether the entries carry the shared step
    counter, orders its group record (``_hyper_values``) and issues its launches (``_launch``).  Gradient accumulation inside the
    update and the device-side schedule are ``FusedAdamW``'s alone: here they raise ``TypeError`` naming the class."""
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")  # state[p]'s names of the flat buffers _exp_avg (and _exp_avg_sq)
    _HAS_STEP = True                         # state[p]["step"]: a 0-d view of the device step counter
    _SCRATCH_WORDS = 2                       # fp32 words of per-call scratch per chunk
    _GROUP_STRUCT = _lib.AdamwGroup          # the by-value record, filled from _hyper_values()

    def _check_lr(self, lr) -> None:
        if isinstance(lr, torch.Tensor):
            raise ValueError(f"mtlora_amd: {type(self).__name__} takes lr as a Python number (it travels in the launch arguments, or with "
                             "capturable=True through push_hyperparameters())")

    def _check_group(self, g: Dict[str, Any]) -> None:
        """ValueError for a param group (the constructor's, or a loaded one) this class cannot run"""

    def _setup(self, params, defaults: Dict[str, Any]) -> None:
        """the constructor behind the subclass's own hyper-parameter checks (``self._capturable`` is set)"""
        name = type(self).__name__
        torch.optim.Optimizer.__init__(self, params, defaults)
        if len(self.param_groups) > _lib.ADAMW_MAX_GROUPS:
            raise ValueError(f"mtlora_amd: {name} supports up to {_lib.ADAMW_MAX_GROUPS} parameter groups")
        self._params: List[torch.Tensor] = []
        group_of: List[int] = []
        for gi, g in enumerate(self.param_groups):
            self._check_group(g)
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"mtlora_amd: {name} updates fp32 parameters only (got {p.dtype}); keep fp32 masters "
                                    "and run the model under autocast")
                self._params.append(p)
                group_of.append(gi)
        _lib.require_gpu(*self._params)
        for p in self._params:
            if not p.is_contiguous():
                raise ValueError(f"mtlora_amd: {name} needs contiguous parameters")
            if p.device != self._params[0].device:
                raise ValueError(f"mtlora_amd: {name} needs all parameters on one device")
        self._build(group_of)

    # ---- device side -------------------------------------------------------------------------------------------------------
    def _build(self, group_of: List[int]) -> None:
        L, dev, nt = _lib.lib(), self._params[0].device, len(self._params)
        self._offsets, total = [], 0
        for p in self._params:
            self._offsets.append(total)
            total += -(-p.numel() // _STATE_ALIGN) * _STATE_ALIGN
        self._group_of = list(group_of)
        self._exp_avg = torch.zeros(max(total, 1), dtype=torch.float32, device=dev)
        # (one flat buffer is enough for a class with one state entry: the table's v column then repeats m, and nothing reads it)
        self._exp_avg_sq = torch.zeros(max(total, 1), dtype=torch.float32, device=dev) if len(self._STATE_KEYS) > 1 else self._exp_avg
        self._ctrl = torch.zeros(_lib.ADAMW_CTRL_WORDS, dtype=torch.float32, device=dev)
        self._has_state = [False] * nt
        numel = (ctypes.c_int64 * nt)(*[p.numel() for p in self._params])
        nc, tb, sb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.mtlora_adamw_sizes(nt, numel, ctypes.byref(nc), ctypes.byref(tb), ctypes.byref(sb)), "adamw_sizes")
        self._n_chunks, self._scratch_bytes = nc.value, sb.value // 2 * self._SCRATCH_WORDS  # (sizes: two words per chunk)
        host = torch.zeros(tb.value // 8, dtype=torch.int64)
        PA = ctypes.c_void_p * nt
        mp, vp = self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr()
        _lib.check(L.mtlora_adamw_table(nt, numel, (ctypes.c_int32 * nt)(*group_of), PA(*[p.data_ptr() for p in self._params]),
                                        PA(*[mp + 4 * o for o in self._offsets]), PA(*[vp + 4 * o for o in self._offsets]),
                                        ctypes.c_void_p(host.data_ptr()), tb.value), "adamw_table")
        self._table = host.to(dev)
        self._param_ptrs = [p.data_ptr() for p in self._params]  # (the table holds them: a re-allocated .data is an error)
        self._grad_ptrs = torch.zeros(nt, dtype=torch.int64, device=dev)
        self._scratch = torch.empty(max(self._scratch_bytes // 4, 1), dtype=torch.float32, device=dev)
        self._groups = (self._GROUP_STRUCT * len(self.param_groups))()
        if self._capturable:
            # the records the kernels read (and, behind them, what the library derives from them): never re-allocated
            self._hyper_dev = torch.zeros(_lib.ADAMW_GROUPS_DEV_BYTES // 8, dtype=torch.float64, device=dev)
            self._hyper_pushed = None  # the values last uploaded
            # a ring of persistent pinned slots, each guarded by the event of the copy that last read it (as data.DeviceLoader's)
            self._hyper_ring = [torch.zeros(_GROUP_WORDS * _lib.ADAMW_MAX_GROUPS, dtype=torch.float64, pin_memory=True)
                                for _ in range(_HYPER_SLOTS)]
            self._hyper_done: List[Optional[torch.cuda.Event]] = [None] * _HYPER_SLOTS
            self._hyper_slot = 0
            # the captured call's gradient pointers: a pinned buffer and a device array of their own, both written ONCE (at
            # capture / in front of the first replay) and alive as long as the optimizer; eager calls never touch them
            self._graph_ptr_host = torch.zeros(nt, dtype=torch.int64, pin_memory=True)
            self._graph_grad_ptrs = torch.zeros(nt, dtype=torch.int64, device=dev)
            self._graph_ptrs: Optional[List[int]] = None
            self._graph_ptrs_sent = True  # (nothing to send yet)
            self._graph_live: List[torch.Tensor] = []
            # the schedule buffer (record, update-call count, lr_used): in place from the start, so that a capture finds it
            self._sched_dev = torch.zeros(_lib.ADAMW_SCHED_DEV_BYTES // 8, dtype=torch.int64, device=dev)
        self._sched = None  # the attached scheduler (capturable only)
        self._sched_loaded: Optional[int] = None  # an update-call count load_state_dict() found and attach_schedule() has yet to use
        self._acc: Optional[torch.Tensor] = None  # gradient accumulation (capturable only): allocated on first use

    def _slot(self, i: int, buf: torch.Tensor) -> torch.Tensor:
        p = self._params[i]
        return buf[self._offsets[i]:self._offsets[i] + p.numel()].view(p.shape)

    def _state_entry(self, i: int, bufs, step, groups) -> Dict[str, Any]:
        """``state[p]`` of parameter i as views of ``bufs`` (the flat buffers, or copies of them) and ``step`` (the counter word);
        ``groups``: the param groups' hyper-parameters, live or packed"""
        s = {"step": step} if self._HAS_STEP else {}
        s.update((k, self._slot(i, b)) for k, b in zip(self._STATE_KEYS, bufs))
        return s

    def _init_state(self, i: int) -> None:
        self.state[self._params[i]] = self._state_entry(i, (self._exp_avg, self._exp_avg_sq), self._ctrl[4], self.param_groups)
        self._has_state[i] = True

    # ---- capturable: hyper-parameters on the device ------------------------------------------------------------------------
    def _hyper_values(self) -> List[float]:
        """the group records, _GROUP_WORDS doubles per group in the record's field order"""
        vals: List[float] = []
        for g in self.param_groups:
            vals += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])]
        return vals

    def _fill_groups(self):
        """the by-value records from ``param_groups`` as of now"""
        vals = self._hyper_values()
        for gi in range(len(self.param_groups)):
            for (name, _), v in zip(self._GROUP_STRUCT._fields_, vals[_GROUP_WORDS * gi:_GROUP_WORDS * (gi + 1)]):
                setattr(self._groups[gi], name, v)
        return self._groups

    def prepare_accumulation(self) -> None:
        raise TypeError(f"mtlora_amd: {type(self).__name__} does not accumulate gradients inside the fused update "
                        "(clip_and_step(accumulation_steps > 1) is FusedAdamW's); let autograd accumulate and call clip_and_step() "
                        "every k-th micro-step")

    def attach_schedule(self, scheduler, num_updates: Optional[int] = None) -> None:
        raise TypeError(f"mtlora_amd: {type(self).__name__} has no device-side schedule (attach_schedule() is FusedAdamW's); set "
                        "param_groups' lr between calls (lr_scheduler.step_update) and, capturable, push_hyperparameters()")

    def push_hyperparameters(self) -> bool:
        """upload ``param_groups``' lr / betas / eps / weight_decay to the device records if they differ from what was pushed
        last (capturable only): one small non-captured copy on the current stream, so call it on the stream that replays, before
        ``replay()``.  The first call after a capture also uploads the captured gradient addresses.  Returns whether
        hyper-parameters were uploaded."""
        if not self._capturable:
            raise RuntimeError(f"mtlora_amd: push_hyperparameters() needs {type(self).__name__}(capturable=True); without it the "
                               "hyper-parameters travel in the launch arguments")
        if not self._graph_ptrs_sent and not torch.cuda.is_current_stream_capturing():
            self._graph_grad_ptrs.copy_(self._graph_ptr_host, non_blocking=True)  # the captured gradient addresses, once
            self._graph_ptrs_sent = True
        vals = self._hyper_values()
        if self._sched is not None and self._hyper_pushed is not None:
            # the kernels take lr from the schedule: a host-side step_update() that moves param_groups["lr"] (for logging) uploads nothing
            vals[0::_GROUP_WORDS] = self._hyper_pushed[0::_GROUP_WORDS]
        if vals == self._hyper_pushed:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mtlora_amd: the hyper-parameters changed inside a graph capture; the upload would be baked into "
                               "the graph -- call push_hyperparameters() before capturing")
        _lib.require_gpu(self._params[0])
        k = self._hyper_slot
        if self._hyper_done[k] is not None:
            self._hyper_done[k].synchronize()  # the copy that last read this slot has finished
        slot = self._hyper_ring[k][:len(vals)]
        slot.copy_(torch.tensor(vals, dtype=torch.float64))
        self._hyper_dev[:len(vals)].copy_(slot, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_done[k] = ev
        self._hyper_slot = (k + 1) % _HYPER_SLOTS
        self._hyper_pushed = vals
        return True

    def bump_versions(self, updated: bool = True) -> None:
        """bump ``_version`` of the parameters the captured ``clip_and_step`` updates -- call it after every replay, so that
        ``MTLoRALinear`` / ``FactorPacker`` copies made from them are seen as stale (the bump inside ``clip_and_step`` is host
        code: it ran at capture, not at replay).  ``updated=False`` after the replay of an accumulating micro-step, which wrote no
        parameter: only the order of calls is checked, no version moves and no cache is invalidated."""
        if self._capturable and self._graph_live:
            if not self._graph_ptrs_sent:  # the replay that just ran read an all-null pointer table: it did nothing but count a step
                raise RuntimeError("mtlora_amd: the captured update was replayed before push_hyperparameters() sent its gradient "
                                   "addresses; call push_hyperparameters() before every replay()")
            if updated:
                torch.autograd.graph.increment_version(self._graph_live)

    def reset_capture(self) -> None:
        """forget the captured gradient addresses, so that ``clip_and_step`` can be captured again (after a capture that was
        aborted, or once the old graph is destroyed).  Replaying a graph captured before this call is an error the optimizer
        cannot detect."""
        if self._capturable:
            self._graph_ptrs, self._graph_live, self._graph_ptrs_sent = None, [], True
            self._ctrl[_lib.ADAMW_CTRL_MICRO:_lib.ADAMW_CTRL_UPDATED + 1].zero_()  # an accumulation cycle starts over

    # ---- the update --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def clip_and_step(self, max_norm: Optional[float] = None, scaler: Optional["LossScaler"] = None,
                      accumulation_steps: int = 1) -> torch.Tensor:
        """unscale (``scaler``) + clip_grad_norm_(``max_norm``) + the class's update + scaler update; returns the total norm of the unscaled
        gradients before clipping as a 0-d device tensor (no ``.item()``, no synchronisation).  ``accumulation_steps`` k > 1: one
        micro-step of gradient accumulation (``FusedAdamW`` only, see there); the norm returned is that of the last update."""
        k = accumulation_steps_of(accumulation_steps)
        if k > 1:
            self.prepare_accumulation()  # (TypeError for a by-value optimizer)
        params, ptrs, live, has = self._params, [], [], self._has_state
        _lib.require_gpu(params[0])
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if not g.is_contiguous():  # (dtype, device and shape are the parameter's: torch checks them when .grad is set)
                raise RuntimeError(f"mtlora_amd: {type(self).__name__} needs dense contiguous gradients (parameter {i}: strides {g.stride()})")
            if p.data_ptr() != self._param_ptrs[i]:
                raise RuntimeError(f"mtlora_amd: parameter {i} was re-allocated after {type(self).__name__} was built; build a new optimizer")
            if not has[i]:
                self._init_state(i)
            ptrs.append(g.data_ptr())
            live.append(p)
        dev = params[0].device
        capturing = self._capturable and torch.cuda.is_current_stream_capturing()
        if capturing:
            if scaler is not None and scaler._scale is None:
                raise RuntimeError("mtlora_amd: the LossScaler must be initialised before a graph capture (one eager step, or "
                                   "what GraphedTrainStep does on construction)")
            if self._graph_ptrs is None:
                self._graph_ptr_host.copy_(torch.tensor(ptrs, dtype=torch.int64))
                self._graph_ptrs, self._graph_live, self._graph_ptrs_sent = ptrs, live, False
            elif ptrs != self._graph_ptrs:  # the device array the earlier graph reads would have to change under it
                raise RuntimeError(f"mtlora_amd: this {type(self).__name__} was already captured with other gradient addresses; one capture "
                                   "per optimizer (reset_capture() once the old graph is gone, or build a new optimizer)")
            # no copy node in the graph: the addresses cannot change from replay to replay, so the array is uploaded ONCE, by an
            # ordinary copy in front of the first replay (push_hyperparameters)
            grad_ptrs = self._graph_grad_ptrs
        else:
            grad_ptrs = self._grad_ptrs
            # pinned staging from torch's caching host allocator: the block is not reused before this copy has run
            host = torch.empty(len(ptrs), dtype=torch.int64, pin_memory=True)
            host.copy_(torch.tensor(ptrs, dtype=torch.int64))
            grad_ptrs.copy_(host, non_blocking=True)
        norm = self._accum_norm if k > 1 else torch.empty((), dtype=torch.float32, device=dev)
        if scaler is not None:
            scaler._lazy_init(dev)
            sc, tr = scaler._scale.data_ptr(), scaler._growth_tracker.data_ptr()
            gf, bf, gint = scaler._growth_factor, scaler._backoff_factor, scaler._growth_interval
        else:
            sc, tr, gf, bf, gint = 0, 0, 2.0, 0.5, 1
        self._launch(grad_ptrs, norm, float(max_norm) if max_norm else 0.0, (sc, tr, gf, bf, gint), k)
        if live:
            torch.autograd.graph.increment_version(live)
        self._opt_called = True  # (what torch's LR schedulers look at to order scheduler.step() after optimizer.step())
        return norm

    def step(self, closure=None):
        """the plain update (no clip, no scaler)"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step()
        return loss

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """the torch counterpart's format (see the class); the tensors are copies (torch's ``load_state_dict`` keeps same-device tensors as they are, and a
        torch optimizer loaded from views would update this optimizer's buffers and step counter in place)"""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for n, v in s.items()}
                       for k, s in sd["state"].items()}
        if self._capturable and self._sched is not None:  # the schedule's position, next to the step counter (torch ignores the key)
            sd["lr_schedule_updates"] = int(self.num_updates().item())
        return sd

    # ---- snapshots (checkpoint.TrainState): the same format from copies of the device buffers, without a synchronisation ------
    def state_tensors(self) -> Dict[str, torch.Tensor]:
        """the device buffers an update call writes, by name: the flat state buffers under their state-entry names, the control block (``[4]`` the step
        count, ``[5]`` the accumulation counter) and, capturable, the schedule buffer (record, count of update calls, lr_used).
        The tensors themselves, not copies; they are never re-allocated."""
        t = dict(zip(self._STATE_KEYS, (self._exp_avg, self._exp_avg_sq)))
        t["ctrl"] = self._ctrl
        if self._capturable:
            t["schedule"] = self._sched_dev
        return t

    def state_meta(self) -> Dict[str, Any]:
        """the host half of ``state_dict()`` as of now: ``param_groups`` in torch's packed form, which parameters have a state
        entry (in ``state``'s order) and whether a schedule is attached.  Reads no device memory."""
        index = {id(p): i for i, p in enumerate(self._params)}
        return {"param_groups": torch.optim.Optimizer.state_dict(self)["param_groups"],
                "order": [index[id(p)] for p in self.state], "scheduled": bool(self._capturable and self._sched is not None)}

    def state_dict_from(self, tensors: Dict[str, torch.Tensor], meta: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """``state_dict()`` as it would read if the device buffers held ``tensors`` -- copies of ``state_tensors()`` on any device,
        for instance views of a pinned snapshot -- and the host half were ``meta`` (``state_meta()``; default: now).  The state
        tensors are VIEWS of ``tensors``; ``"lr_schedule_updates"`` is read from ``tensors["schedule"]``."""
        meta = self.state_meta() if meta is None else meta
        bufs, step = [tensors[k] for k in self._STATE_KEYS], tensors["ctrl"][4]
        sd = {"state": {i: self._state_entry(i, bufs, step, meta["param_groups"]) for i in meta["order"]},
              "param_groups": meta["param_groups"]}
        if meta["scheduled"]:
            sd["lr_schedule_updates"] = int(tensors["schedule"][_lib.ADAMW_SCHED_COUNT_OFFSET // 8].item())
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        step = uniform_step(state_dict["state"], type(self).__name__) if self._HAS_STEP else 0.0  # before anything is touched
        for g in state_dict["param_groups"]:
            self._check_group(g)
        super().load_state_dict(state_dict)
        index = {id(p): i for i, p in enumerate(self._params)}
        loaded = dict(self.state)
        self.state.clear()
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        self._has_state = [False] * len(self._params)
        for p, s in loaded.items():
            i = index[id(p)]
            for k, buf in zip(self._STATE_KEYS, (self._exp_avg, self._exp_avg_sq)):
                if s[k] is not None:  # (torch SGD without momentum keeps momentum_buffer: None)
                    self._slot(i, buf).copy_(s[k])
            self._init_state(i)
        self._ctrl.zero_()
        self._ctrl[4] = step
        if self._capturable and "lr_schedule_updates" in state_dict:  # (a state without the key loads as it always did)
            n = int(state_dict["lr_schedule_updates"])
            if self._sched is not None:
                self._sched_dev[_lib.ADAMW_SCHED_COUNT_OFFSET // 8] = n
            else:
                self._sched_loaded = n  # the next attach_schedule() starts from it
        for g in self.param_groups:
            if "capturable" in g:
                g["capturable"] = self._capturable  # (a property of this object's buffers, not of the checkpoint)
        if self._capturable:
            for p in self._graph_live:  # the captured update keeps writing these slices: they keep their (now zero) state entries
                if not self._has_state[index[id(p)]]:
                    self._init_state(index[id(p)])


class FusedAdamW(FusedOptimizer):
    """``torch.optim.AdamW`` (decoupled weight decay) whose ``step`` is the multi-tensor HIP update.

    * ``step()`` is plain AdamW; ``clip_and_step(max_norm, scaler)`` is the fused clip_grad_norm_ + unscale + AdamW + scaler update.
    * ``exp_avg`` / ``exp_avg_sq`` live in two flat fp32 buffers; ``state[p]`` holds views into them and a 0-d view of the single
      device step counter.  A parameter gets its ``state`` entry the first time it has a gradient, as in torch.
    * ``state_dict()`` / ``load_state_dict()`` use torch AdamW's format, so checkpoints interchange with ``torch.optim.AdamW``
      (``state_dict()`` returns copies, not views).  The one restriction: all parameters share ONE step counter.
    * A gradient holding inf / nan skips the whole step on the device (parameters, state and the counter stay bitwise unchanged),
      with or without a scaler; the returned norm is then non-finite.
    * Every parameter that had a gradient gets its ``_version`` bumped after each call -- the kernels write through raw pointers,
      and ``MTLoRALinear`` / ``FactorPacker`` judge freshness by ``_version``.  This includes skipped steps (the skip is decided
      on the device; the host cannot know).
    * ``capturable=True``: ``clip_and_step`` may be captured in a HIP graph (``torch.cuda.graph``,
      ``mtl_harness.GraphedTrainStep``) and replayed.  The hyper-parameters then live in a device buffer the kernels read at run
      time (``mtlora_adamw_update_dev``; bit-identical to the by-value path), so a replay follows ``param_groups``: set them,
      call ``push_hyperparameters()`` (an ordinary copy on the current stream, only if something changed), replay.  After a
      replay call ``bump_versions()`` -- the version bump above is host code and is not replayed.  Hyper-parameters are NOT
      validated on this path: a value the by-value path rejects (negative lr, beta >= 1, nan) makes the device skip the step and
      return a nan norm.  Inside a capture the scaler must already be initialised and the hyper-parameters pushed; the gradient
      addresses of the capture go into a device array of their own, uploaded once by the first ``push_hyperparameters()`` after
      the capture (so that call is needed before the first replay even if no value changed), and ONE set of gradient addresses
      can be captured per optimizer (eager calls between replays use buffers of their own).
    * ``clip_and_step(..., accumulation_steps=k)`` with k > 1 (capturable only) is ONE MICRO-STEP of gradient accumulation
      (``mtlora_adamw_accum_update_dev``; main.py:347-353): the gradients are added into a persistent fp32 accumulator the size of
      all parameters (allocated at the first such call, or by ``prepare_accumulation()``; never zeroed: a cycle's first micro-step
      overwrites it) and a device counter decides whether this call is the cycle's k-th, the only one that clips, steps and
      updates the scaler.  The caller zeroes the gradients after EVERY call (they have been consumed), does not divide the loss by
      k, and a parameter has a gradient in all of a cycle's micro-steps or in none.  The returned norm is a persistent 0-d tensor
      that keeps the last update's value.  The accumulator and the counter are not part of ``state_dict()`` (the reference does
      not checkpoint ``.grad`` either); ``load_state_dict()`` and ``reset_capture()`` return the counter to 0.
    * ``attach_schedule(scheduler)`` (capturable only) moves the learning-rate schedule onto the device
      (``mtlora_adamw_sched_update_dev``): every update call then takes each group's lr from the schedule, at a count ``u`` of
      update calls the kernels keep themselves, and ``lr_scheduler.step_update`` has nothing left to do -- a replayed step needs
      no ``push_hyperparameters()`` upload for the lr.  Update call n uses ``scheduler._get_lr(max(n - 1, 0))``: the reference
      steps its scheduler AFTER the optimizer (main.py:350-353), so update 0 runs at the constructor's value, which is
      ``_get_lr(0)``, and update n at what ``step_update(n - 1)`` set.  This reproduces the reference whenever ``num_steps %
      ACCUMULATION_STEPS == 0`` (otherwise its ``(epoch * num_steps + idx) // k`` repeats a count at an epoch boundary).  ``u``
      counts CALLS: a call skipped for inf / nan advances it and not the Adam step.  ``lr_used()`` / ``num_updates()`` are device
      views for logging; ``state_dict()`` carries ``u`` under ``"lr_schedule_updates"`` while a schedule is attached.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, maximize: bool = False, capturable: bool = False):
        if amsgrad or maximize:
            raise ValueError("mtlora_amd: FusedAdamW supports neither amsgrad nor maximize")
        self._check_lr(lr)
        self._capturable = bool(capturable)
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"mtlora_amd: invalid AdamW hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        # torch AdamW's group keys, so that the two state_dict formats interchange
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=self._capturable, differentiable=False, fused=None, decoupled_weight_decay=True)
        self._setup(params, defaults)

    def _check_group(self, g: Dict[str, Any]) -> None:
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("mtlora_amd: FusedAdamW supports neither amsgrad nor maximize")

    def _launch(self, grad_ptrs: torch.Tensor, norm: torch.Tensor, max_norm: float, scaler_args, k: int) -> None:
        params = self._params
        sc, tr, gf, bf, gint = scaler_args
        if self._capturable and self._sched is not None:  # the lr comes from the schedule buffer, for any k
            self.push_hyperparameters()  # (betas / eps / weight decay, on change)
            acc, off = (self._acc.data_ptr(), self._acc_offsets.data_ptr()) if k > 1 else (0, 0)
            _lib.check(_lib.lib().mtlora_adamw_sched_update_dev(
                self._table.data_ptr(), grad_ptrs.data_ptr(), len(params), self._n_chunks, self._hyper_dev.data_ptr(),
                len(self.param_groups), max_norm, self._ctrl.data_ptr(), norm.data_ptr(), sc, tr, gf,
                bf, gint, self._scratch.data_ptr(), self._scratch_bytes, acc, off, k, self._sched_dev.data_ptr(),
                _lib.stream_ptr()), "adamw_sched_update_dev")
        elif k > 1:
            self.push_hyperparameters()
            _lib.check(_lib.lib().mtlora_adamw_accum_update_dev(
                self._table.data_ptr(), grad_ptrs.data_ptr(), len(params), self._n_chunks, self._hyper_dev.data_ptr(),
                len(self.param_groups), max_norm, self._ctrl.data_ptr(), norm.data_ptr(), sc, tr, gf,
                bf, gint, self._scratch.data_ptr(), self._scratch_bytes, self._acc.data_ptr(), self._acc_offsets.data_ptr(), k,
                _lib.stream_ptr()), "adamw_accum_update_dev")
        elif self._capturable:
            self.push_hyperparameters()  # (uploads only on change; raises if that happens inside a capture)
            _lib.check(_lib.lib().mtlora_adamw_update_dev(
                self._table.data_ptr(), grad_ptrs.data_ptr(), len(params), self._n_chunks, self._hyper_dev.data_ptr(),
                len(self.param_groups), max_norm, self._ctrl.data_ptr(), norm.data_ptr(), sc, tr, gf,
                bf, gint, self._scratch.data_ptr(), self._scratch_bytes, _lib.stream_ptr()), "adamw_update_dev")
        else:
            _lib.check(_lib.lib().mtlora_adamw_update(
                self._table.data_ptr(), grad_ptrs.data_ptr(), len(params), self._n_chunks, self._fill_groups(), len(self.param_groups),
                max_norm, self._ctrl.data_ptr(), norm.data_ptr(), sc, tr, gf, bf, gint,
                self._scratch.data_ptr(), self._scratch_bytes, _lib.stream_ptr()), "adamw_update")

    def prepare_accumulation(self) -> None:
        """allocate what ``clip_and_step(accumulation_steps > 1)`` needs -- the fp32 accumulator (as many elements as all parameters
        together; NOT zeroed), its offset table and the persistent norm word -- so that a graph capture finds them in place"""
        if not self._capturable:
            raise TypeError("mtlora_amd: gradient accumulation inside the fused update needs FusedAdamW(capturable=True); with the "
                            "by-value optimizer let autograd accumulate and call clip_and_step() every k-th micro-step")
        if self._acc is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mtlora_amd: the accumulator must exist before a graph capture; call prepare_accumulation() first")
        nt, dev = len(self._params), self._params[0].device
        numel = (ctypes.c_int64 * nt)(*[p.numel() for p in self._params])
        offs, total = torch.zeros(nt, dtype=torch.int64), ctypes.c_int64()
        _lib.check(_lib.lib().mtlora_adamw_accum_layout(nt, numel, ctypes.cast(offs.data_ptr(), ctypes.POINTER(ctypes.c_int64)),
                                                        ctypes.byref(total)), "adamw_accum_layout")
        self._acc_offsets = offs.to(dev)
        self._accum_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._acc = torch.empty(max(total.value, 4), dtype=torch.float32, device=dev)

    # ---- capturable: the learning-rate schedule on the device ---------------------------------------------------------------
    def _schedule_record(self, scheduler) -> "_lib.LrSchedule":
        """``scheduler`` (one of lr_scheduler's four classes, counted in updates) as the record the kernels read; ValueError for
        what they would reject"""
        from . import lr_scheduler as S
        kinds = ((S.CosineLRScheduler, _lib.LR_COSINE), (S.StepLRScheduler, _lib.LR_STEP), (S.LinearLRScheduler, _lib.LR_LINEAR),
                 (S.MultiStepLRScheduler, _lib.LR_MULTISTEP))
        kind = next((k for c, k in kinds if isinstance(scheduler, c)), None)
        if kind is None:
            raise TypeError("mtlora_amd: attach_schedule() takes a scheduler of mtlora_amd.lr_scheduler (cosine, step, linear or "
                            f"multistep), got {type(scheduler).__name__}")
        if scheduler.t_in_epochs:
            raise ValueError("mtlora_amd: the device-side schedule counts update calls; build the scheduler with t_in_epochs=False")
        n = len(self.param_groups)
        if len(scheduler.base_values) != n:
            raise ValueError(f"mtlora_amd: the scheduler has {len(scheduler.base_values)} base values, the optimizer {n} groups")
        r = _lib.LrSchedule()
        r.kind, r.warmup_t, r.warmup_lr_init = kind, int(scheduler.warmup_t), float(scheduler.warmup_lr_init)
        for g, v in enumerate(scheduler.base_values):
            r.base_lr[g] = float(v)
        if kind == _lib.LR_COSINE:
            if (scheduler.cycle_mul, scheduler.cycle_decay, scheduler.cycle_limit, scheduler.k_decay) != (1, 1, 1, 1):
                raise ValueError("mtlora_amd: the device-side cosine schedule is one cycle without decay")
            r.t_initial, r.lr_min, r.warmup_prefix = int(scheduler.t_initial), float(scheduler.lr_min), int(bool(scheduler.warmup_prefix))
        elif kind == _lib.LR_STEP:
            r.decay_t, r.decay_rate = int(scheduler.decay_t), float(scheduler.decay_rate)
        elif kind == _lib.LR_LINEAR:
            r.t_initial, r.lr_min_rate = int(scheduler.t_initial), float(scheduler.lr_min_rate)
        else:
            ms = [int(m) for m in scheduler.milestones]
            if len(ms) > _lib.LR_MAX_MILESTONES:
                raise ValueError(f"mtlora_amd: the device-side multistep schedule holds up to {_lib.LR_MAX_MILESTONES} milestones, got {len(ms)}")
            r.gamma, r.n_milestones = float(scheduler.gamma), len(ms)
            for i, m in enumerate(ms):
                r.milestones[i] = m
        for name in ("warmup_t", "t_initial", "decay_t"):  # counts the kernels hold as integers
            if hasattr(scheduler, name) and int(getattr(scheduler, name)) != getattr(scheduler, name):
                raise ValueError(f"mtlora_amd: the device-side schedule needs an integer {name}, got {getattr(scheduler, name)!r}")
        if _lib.lib().mtlora_lr_schedule_check(ctypes.byref(r), n) != 0:
            raise ValueError("mtlora_amd: this schedule cannot run on the device (a nan or negative value, t_initial <= 0 where it "
                             "divides, milestones that are not ascending, below 1 or inside the warm-up): "
                             f"{ {k: v for k, v in scheduler.state_dict().items() if not k.startswith('_')} }")
        return r

    def attach_schedule(self, scheduler, num_updates: Optional[int] = None) -> None:
        """run ``scheduler`` on the device from now on (see the class): the record is validated, uploaded with an ordinary copy,
        and the count of update calls set to ``num_updates`` -- by default the count ``load_state_dict()`` found in the checkpoint
        if there was one, else what the scheduler last saw (0 for a fresh one, n + 1 after ``step_update(n)`` or after its
        ``load_state_dict`` of such a state).  Attach BEFORE capturing ``clip_and_step``: a graph keeps the entry point of its capture."""
        if not self._capturable:
            raise TypeError("mtlora_amd: attach_schedule() needs FusedAdamW(capturable=True); a by-value optimizer takes its lr "
                            "from param_groups at every call (lr_scheduler.step_update)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mtlora_amd: attach_schedule() inside a graph capture: the upload would be baked into the graph -- "
                               "attach the schedule before capturing")
        if self._graph_ptrs is not None:
            raise RuntimeError("mtlora_amd: clip_and_step was already captured without this schedule; attach it before the capture "
                               "(or reset_capture() once the old graph is gone)")
        rec = self._schedule_record(scheduler)
        if num_updates is None:
            num_updates = self._sched_loaded if self._sched_loaded is not None else int(getattr(scheduler, "num_updates_seen", 0))
        if isinstance(num_updates, bool) or int(num_updates) != num_updates or num_updates < 0:
            raise ValueError(f"mtlora_amd: num_updates must be an integer >= 0, got {num_updates!r}")
        _lib.require_gpu(self._params[0])
        host = torch.zeros(_lib.ADAMW_SCHED_DEV_BYTES // 8, dtype=torch.int64)
        ctypes.memmove(host.data_ptr(), ctypes.byref(rec), ctypes.sizeof(rec))
        host[_lib.ADAMW_SCHED_COUNT_OFFSET // 8] = int(num_updates)
        self._sched_dev.copy_(host)  # (lr_used starts at 0.0; the first update call writes it)
        self._sched, self._sched_loaded = scheduler, None

    def detach_schedule(self) -> None:
        """back to the group records' lr (``param_groups`` through ``push_hyperparameters()``) from the next call on; the count
        and ``lr_used`` keep their last values.  As ``attach_schedule``: not under a capture, not after one."""
        if self._sched is None:
            return
        if torch.cuda.is_current_stream_capturing() or self._graph_ptrs is not None:
            raise RuntimeError("mtlora_amd: detach_schedule() cannot change a captured clip_and_step; reset_capture() first, once "
                               "the graph is gone")
        self._sched = None
        self._hyper_pushed = None  # the lr in the device records is whatever was pushed before the schedule took over: push again

    def _need_schedule(self) -> None:
        if not self._capturable or self._sched is None:
            raise RuntimeError("mtlora_amd: no schedule is attached (FusedAdamW(capturable=True).attach_schedule(scheduler))")

    def lr_used(self) -> torch.Tensor:
        """the learning rates the last update call used, one double per param group: a view of device memory, no synchronisation"""
        self._need_schedule()
        at = _lib.ADAMW_SCHED_LR_OFFSET // 8
        return self._sched_dev.view(torch.float64)[at:at + len(self.param_groups)]

    def num_updates(self) -> torch.Tensor:
        """the number of update calls made so far (skipped ones included), a 0-d int64 view of device memory"""
        self._need_schedule()
        return self._sched_dev[_lib.ADAMW_SCHED_COUNT_OFFSET // 8]


class FusedSGD(FusedOptimizer):
    """``torch.optim.SGD(momentum, dampening=0, weight_decay, nesterov)`` -- the reference's ``sgd`` (optimizer.py:56 builds it with
    ``nesterov=True``) -- as THREE launches (norm, finish, step; ``mtlora_sgd_update`` / ``mtlora_sgd_update_dev``), with everything
    ``FusedOptimizer`` carries: the fused clip + unscale, the inf / nan skip on the device, ``LossScaler``, the capturable form.

        g' = g + wd p (coupled L2);  buf = mu buf + g';  p -= lr (g' + mu buf) if nesterov else lr buf

    with g the unscaled, clipped gradient.  The buffers start at zero, which is torch's first step (``buf = g'``) because dampening
    is 0; ``momentum=0`` is plain SGD, and the buffer is then neither read nor written.  ``dampening != 0`` and ``maximize`` are a
    ``ValueError``.  ``state_dict()`` / ``load_state_dict()`` use torch SGD's format -- a ``momentum_buffer`` per parameter that has
    had a gradient (``None`` without momentum), no step entry, torch's group keys -- so checkpoints interchange with
    ``torch.optim.SGD`` both ways.  ``sgd_update_torch`` states the arithmetic in plain torch.

    Out of scope: ``clip_and_step(accumulation_steps=k > 1)``, ``attach_schedule()`` and therefore
    ``GraphedTrainStep(accumulation_steps > 1 | lr_scheduler=)`` -- each raises ``TypeError`` naming this class.  Accumulate with
    ``train_step(update_grad=False)``, and move the lr through ``param_groups`` (+ ``push_hyperparameters()`` when capturable)."""
    _STATE_KEYS = ("momentum_buffer",)
    _HAS_STEP = False
    _GROUP_STRUCT = _lib.SgdGroup

    def __init__(self, params, lr: float, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, capturable: bool = False, *, maximize: bool = False):
        self._check_lr(lr)
        self._capturable = bool(capturable)
        if not 0.0 <= lr or not 0.0 <= momentum or not 0.0 <= weight_decay:
            raise ValueError(f"mtlora_amd: invalid SGD hyper-parameters lr={lr} momentum={momentum} weight_decay={weight_decay}")
        # torch SGD's group keys, so that the two state_dict formats interchange
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                        maximize=bool(maximize), foreach=None, differentiable=False, fused=None)
        self._check_group(defaults)
        self._setup(params, defaults)

    def _check_group(self, g: Dict[str, Any]) -> None:
        if g.get("dampening") or g.get("maximize"):
            raise ValueError("mtlora_amd: FusedSGD supports neither dampening != 0 nor maximize")
        if g.get("nesterov") and not g.get("momentum", 0.0) > 0.0:
            raise ValueError("mtlora_amd: FusedSGD: Nesterov momentum requires a momentum (as torch.optim.SGD)")

    def _hyper_values(self) -> List[float]:
        vals: List[float] = []
        for g in self.param_groups:
            vals += [float(g["lr"]), float(g["momentum"]), 1.0 if g["nesterov"] else 0.0, 0.0, float(g["weight_decay"])]
        return vals

    def _state_entry(self, i: int, bufs, step, groups) -> Dict[str, Any]:
        if not groups[self._group_of[i]]["momentum"]:
            return {"momentum_buffer": None}  # as torch: no momentum, no buffer
        return super()._state_entry(i, bufs, step, groups)

    def _launch(self, grad_ptrs: torch.Tensor, norm: torch.Tensor, max_norm: float, scaler_args, k: int) -> None:
        head = (self._table.data_ptr(), grad_ptrs.data_ptr(), len(self._params), self._n_chunks)
        tail = (max_norm, self._ctrl.data_ptr(), norm.data_ptr(), *scaler_args, self._scratch.data_ptr(), self._scratch_bytes,
                _lib.stream_ptr())
        if self._capturable:
            self.push_hyperparameters()  # (uploads only on change; raises if that happens inside a capture)
            _lib.check(_lib.lib().mtlora_sgd_update_dev(*head, self._hyper_dev.data_ptr(), len(self.param_groups), *tail),
                       "sgd_update_dev")
        else:
            _lib.check(_lib.lib().mtlora_sgd_update(*head, self._fill_groups(), len(self.param_groups), *tail), "sgd_update")


class FusedLAMB(FusedOptimizer):
    """LAMB by the algorithm of apex's ``FusedLAMB`` -- the reference's ``fused_lamb`` (optimizer.py:63), which has no torch
    implementation -- with the arguments the reference leaves at their defaults (``bias_correction``, ``grad_averaging`` and
    ``adam_w_mode`` are accepted only as ``True``, ``amsgrad`` only as ``False``), as FOUR launches (norm, finish, moments +
    per-chunk partials, apply; ``mtlora_lamb_update`` / ``mtlora_lamb_update_dev``).  With g the unscaled gradient after
    ``clip_and_step``'s own ``max_norm`` clip and n the global norm of those g:

        c = n / max_grad_norm if n > max_grad_norm else 1 (``max_grad_norm`` <= 0 or None: never);  g = g / c
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd p
        ratio = lr |p| / |u| if (wd != 0 or use_nvlamb) and |p| != 0 and |u| != 0 else lr, per tensor;  p -= ratio u

    t is ONE step count for all parameters, as ``FusedAdamW``'s.  u is not stored: the fourth launch forms it again from the
    stored m, v and the still unmodified p.  The per-tensor norms are per-chunk partial sums added in a fixed order (no float
    atomics): runs are bit-reproducible.  ``max_grad_norm`` and ``use_nvlamb`` are read from the defaults (they are launch
    arguments: a captured call keeps those of its capture); lr, betas, eps and weight_decay per group.  ``state_dict()`` has
    ``FusedAdamW``'s layout (``step``, ``exp_avg``, ``exp_avg_sq``) with LAMB's group keys; interchange with apex is not claimed.
    ``lamb_update_torch`` states the arithmetic in plain torch.

    Out of scope: ``clip_and_step(accumulation_steps=k > 1)``, ``attach_schedule()`` and therefore
    ``GraphedTrainStep(accumulation_steps > 1 | lr_scheduler=)`` -- each raises ``TypeError`` naming this class."""
    _SCRATCH_WORDS = 4  # per chunk: the gradient partial and flag, and the partials of |p|^2 and |u|^2

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01,
                 max_grad_norm: Optional[float] = 1.0, use_nvlamb: bool = False, capturable: bool = False, *,
                 bias_correction: bool = True, grad_averaging: bool = True, adam_w_mode: bool = True, amsgrad: bool = False):
        self._check_lr(lr)
        self._capturable = bool(capturable)
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"mtlora_amd: invalid LAMB hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if max_grad_norm is not None and max_grad_norm != max_grad_norm:
            raise ValueError("mtlora_amd: FusedLAMB max_grad_norm is nan")
        defaults = dict(lr=lr, bias_correction=bias_correction, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        amsgrad=amsgrad, adam_w_mode=adam_w_mode, grad_averaging=grad_averaging,
                        max_grad_norm=None if max_grad_norm is None else float(max_grad_norm), use_nvlamb=bool(use_nvlamb),
                        capturable=self._capturable)
        self._check_group(defaults)
        self._setup(params, defaults)

    def _check_group(self, g: Dict[str, Any]) -> None:
        if not (g.get("bias_correction", True) and g.get("grad_averaging", True) and g.get("adam_w_mode", True)) or g.get("amsgrad"):
            raise ValueError("mtlora_amd: FusedLAMB runs bias_correction=True, grad_averaging=True, adam_w_mode=True and "
                             "amsgrad=False only")

    def _launch(self, grad_ptrs: torch.Tensor, norm: torch.Tensor, max_norm: float, scaler_args, k: int) -> None:
        head = (self._table.data_ptr(), grad_ptrs.data_ptr(), len(self._params), self._n_chunks)
        tail = (max_norm, float(self.defaults["max_grad_norm"] or 0.0), int(bool(self.defaults["use_nvlamb"])), self._ctrl.data_ptr(),
                norm.data_ptr(), *scaler_args, self._scratch.data_ptr(), self._scratch_bytes, _lib.stream_ptr())
        if self._capturable:
            self.push_hyperparameters()  # (uploads only on change; raises if that happens inside a capture)
            _lib.check(_lib.lib().mtlora_lamb_update_dev(*head, self._hyper_dev.data_ptr(), len(self.param_groups), *tail),
                       "lamb_update_dev")
        else:
            _lib.check(_lib.lib().mtlora_lamb_update(*head, self._fill_groups(), len(self.param_groups), *tail), "lamb_update")


# ---- the two updates in plain torch: what the kernels compute, in any dtype, on any device ---------------------------------------
def _unscale_and_clip(grads, dtype, max_norm, scale):
    """(norm of the unscaled gradients, found_inf, clip coefficient, 1 / scale) as k_optim_finish forms them"""
    live = [g for g in grads if g is not None]
    inv = 1.0 / float(scale)
    total = torch.sqrt(sum((g.to(dtype) ** 2).sum() for g in live)) * inv if live else torch.zeros((), dtype=dtype)
    found = any(not torch.isfinite(g).all().item() for g in live)
    coef = torch.clamp(float(max_norm) / (total + 1e-6), max=1.0) if max_norm and max_norm > 0 else torch.ones_like(total)
    return total, found, coef, inv


@torch.no_grad()
def sgd_update_torch(params, grads, bufs, group_of, groups, max_norm=None, scale: float = 1.0):
    """``FusedSGD.clip_and_step`` restated: ``params`` and ``bufs`` (momentum buffers, zero before the first step) are updated in
    place, in their own dtype; ``grads[i]`` is the stored gradient (still multiplied by ``scale``) or None; ``groups[group_of[i]]``
    holds ``lr``, ``momentum``, ``weight_decay``, ``nesterov``.  Returns ``(norm, skipped)``: the norm of the unscaled gradients
    before clipping, and whether an inf / nan skipped the step (nothing is written then)."""
    dtype = params[0].dtype
    total, found, coef, inv = _unscale_and_clip(grads, dtype, max_norm, scale)
    if found:
        return total, True
    gmul = coef * inv
    for p, g, buf, gi in zip(params, grads, bufs, group_of):
        if g is None:
            continue
        h = groups[gi]
        lr, mu, wd = float(h["lr"]), float(h["momentum"]), float(h["weight_decay"])
        g = g.to(dtype) * gmul + wd * p
        if mu == 0.0:
            p.sub_(lr * g)
            continue
        buf.mul_(mu).add_(g)
        p.sub_(lr * (g + mu * buf if h["nesterov"] else buf))
    return total, False


@torch.no_grad()
def lamb_update_torch(params, grads, exp_avgs, exp_avg_sqs, group_of, groups, state, max_norm=None, scale: float = 1.0,
                      max_grad_norm: Optional[float] = 1.0, use_nvlamb: bool = False):
    """``FusedLAMB.clip_and_step`` restated (see the class for the formulas): ``params``, ``exp_avgs`` and ``exp_avg_sqs`` are
    updated in place in their own dtype, ``state["step"]`` (an int, the shared count) moves unless the step is skipped;
    ``groups[group_of[i]]`` holds ``lr``, ``betas``, ``eps``, ``weight_decay``.  Returns a dict: ``norm`` (unscaled, before any clip),
    ``skipped``, ``clip`` (LAMB's own divisor c) and ``ratio`` (per parameter: what multiplied u; None without a gradient)."""
    dtype = params[0].dtype
    total, found, coef, inv = _unscale_and_clip(grads, dtype, max_norm, scale)
    out = {"norm": total, "skipped": found, "clip": None, "ratio": [None] * len(params)}
    if found:
        return out
    n2 = total * coef  # the norm of the gradients after the max_norm clip
    c = n2 / float(max_grad_norm) if (max_grad_norm and max_grad_norm > 0 and n2 > max_grad_norm) else torch.ones_like(total)
    out["clip"] = c
    gmul = coef * inv / c
    state["step"] = t = int(state.get("step", 0)) + 1
    for i, (p, g, m, v, gi) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs, group_of)):
        if g is None:
            continue
        h = groups[gi]
        lr, (b1, b2), eps, wd = float(h["lr"]), h["betas"], float(h["eps"]), float(h["weight_decay"])
        g = g.to(dtype) * gmul
        m.mul_(b1).add_((1.0 - b1) * g)
        v.mul_(b2).add_((1.0 - b2) * g * g)
        u = (m / (1.0 - b1 ** t)) / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps) + wd * p
        pn, un = torch.sqrt((p * p).sum()), torch.sqrt((u * u).sum())
        ratio = lr * (pn / un) if ((wd != 0.0 or use_nvlamb) and pn != 0 and un != 0) else torch.full_like(pn, lr)
        out["ratio"][i] = ratio
        p.sub_(ratio * u)
    return out


class LossScaler:
    """The reference's ``NativeScalerWithGradNormCount`` (utils.py:348-375) for ``FusedAdamW``: the scale and the growth tracker
    live on the device and are read / updated by the optimizer's kernels (``torch.amp.GradScaler`` semantics: a step with inf /
    nan gradients is skipped and the scale backs off; ``growth_interval`` good steps in a row grow it).  ``state_dict`` has
    ``GradScaler``'s keys."""
    state_dict_key = "amp_scaler"

    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        if growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1:
            raise ValueError("mtlora_amd: LossScaler needs growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._scale: Optional[torch.Tensor] = None
        self._growth_tracker: Optional[torch.Tensor] = None

    def _lazy_init(self, device) -> None:
        if self._scale is None:
            _lib.require_gpu(torch.empty(0, device=device))
            self._scale = torch.full((), self._init_scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((), self._init_growth_tracker, dtype=torch.int32, device=device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        self._lazy_init(loss.device)
        return loss * self._scale.to(loss.dtype)

    def get_scale(self) -> float:
        return self._init_scale if self._scale is None else float(self._scale.item())

    def __call__(self, loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        """scaled backward, then (``update_grad``) the fused update; returns the gradient norm, or None when the gradients are
        only accumulated.  ``parameters`` is accepted for the reference's signature: what is clipped is the optimizer's own set."""
        if not isinstance(optimizer, FusedOptimizer):
            raise TypeError("mtlora_amd: LossScaler drives FusedAdamW only, or its siblings FusedSGD / FusedLAMB "
                            f"(build_optimizer(impl='hip')); got {type(optimizer).__name__}")
        self.scale(loss).backward(create_graph=create_graph)
        return optimizer.clip_and_step(max_norm=clip_grad, scaler=self) if update_grad else None

    def state_dict(self) -> Dict[str, Any]:
        tracker = self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def device_words(self) -> Optional[Dict[str, torch.Tensor]]:
        """the two device words the optimizer's kernels update (the tensors themselves), or None before the first use"""
        return None if self._scale is None else {"scale": self._scale, "growth_tracker": self._growth_tracker}

    def state_dict_from(self, words: Optional[Dict[str, torch.Tensor]]) -> Dict[str, Any]:
        """``state_dict()`` as it would read if the device words held ``words`` (copies of ``device_words()`` on any device; None:
        the scaler was not initialised when they were taken)"""
        scale = self._init_scale if words is None else float(words["scale"].item())
        tracker = self._init_growth_tracker if words is None else int(words["growth_tracker"].item())
        return {"scale": scale, "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        if len(state_dict) == 0:
            raise RuntimeError("mtlora_amd: the source state dict is empty, possibly because it was saved from a disabled GradScaler")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval, self._init_growth_tracker = int(state_dict["growth_interval"]), int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)
