"""The learning-rate schedules of the reference (lr_scheduler.py: ``build_scheduler``, ``LinearLRScheduler``,
``MultiStepLRScheduler``, and the two timm 0.9.2 classes it imports, ``CosineLRScheduler`` / ``StepLRScheduler``) without timm: pure
Python, no dependency beyond the optimizer's ``param_groups``.

    lr_scheduler = build_scheduler(config, optimizer, len(data_loader_train))
    ...
    lr_scheduler.step_update((epoch * num_steps + idx) // config.TRAIN.ACCUMULATION_STEPS)      # main.py:350-353

``Scheduler`` is the subset of ``timm.scheduler.scheduler.Scheduler`` the reference uses: the field is ``lr``, ``initial_lr`` is
written into every param group at construction and ``base_values`` read from it, ``step(epoch)`` / ``step_update(num_updates)``
write ``param_groups``, ``state_dict()`` is every attribute but the optimizer.  LR noise is not implemented (the reference never
asks for it): any noise argument other than ``None`` raises.

The same schedules run ON THE DEVICE inside the fused update once ``optim.FusedAdamW.attach_schedule(scheduler)`` has uploaded
them (csrc/optim.hip): the kernels then count the update calls themselves and the host has nothing to do between two replays of
a captured step.  ``num_updates_seen`` is what that call starts the device counter from.

Values, for a base value ``v`` (``t_in_epochs=False``: ``get_update_values(t) = _get_lr(t)``), in exactly this expression order --
the device code forms the same IEEE operations, so warm-up and the linear kind agree with it bit for bit:
    warm-up (all)   t < warmup_t:  warmup_lr_init + t * s,  s = (v - warmup_lr_init) / warmup_t  (formed once, at construction)
    cosine          t -= warmup_t if warmup_prefix;  i = t // t_initial;  t_curr = t - t_initial * i;
                    lr_min + 0.5 * (v - lr_min) * (1 + cos(pi * t_curr / t_initial)) if i < cycle_limit else lr_min
    step            v * decay_rate ** (t // decay_t)
    linear          t -= warmup_t;  total = t_initial - warmup_t;  v - (v - v * lr_min_rate) * (t / total)
    multistep       v * gamma ** bisect_right(milestones, t)
"""
from __future__ import annotations

import bisect
import math
from typing import Any, Dict, List, Optional

__all__ = ["build_scheduler", "Scheduler", "CosineLRScheduler", "StepLRScheduler", "LinearLRScheduler", "MultiStepLRScheduler"]


def build_scheduler(config, optimizer, n_iter_per_epoch):
    """the scheduler ``config.TRAIN.LR_SCHEDULER.NAME`` asks for, counted in updates (``t_in_epochs=False``); None for a name
    that is none of cosine / linear / step / multistep"""
    train = config.TRAIN
    num_steps = int(train.EPOCHS * n_iter_per_epoch)
    warmup_steps = int(train.WARMUP_EPOCHS * n_iter_per_epoch)
    name = train.LR_SCHEDULER.NAME
    common = dict(warmup_lr_init=train.WARMUP_LR, warmup_t=warmup_steps, t_in_epochs=False)
    if name == "cosine":
        prefix = train.LR_SCHEDULER.WARMUP_PREFIX
        return CosineLRScheduler(optimizer, t_initial=(num_steps - warmup_steps) if prefix else num_steps, lr_min=train.MIN_LR,
                                 cycle_limit=1, warmup_prefix=prefix, **common)
    if name == "linear":
        return LinearLRScheduler(optimizer, t_initial=num_steps, lr_min_rate=0.01, **common)
    if name == "step":
        return StepLRScheduler(optimizer, decay_t=int(train.LR_SCHEDULER.DECAY_EPOCHS * n_iter_per_epoch),
                               decay_rate=train.LR_SCHEDULER.DECAY_RATE, **common)
    if name == "multistep":
        return MultiStepLRScheduler(optimizer, milestones=[i * n_iter_per_epoch for i in train.LR_SCHEDULER.MULTISTEPS],
                                    gamma=train.LR_SCHEDULER.GAMMA, **common)
    return None


class Scheduler:
    """parameter-group scheduler base: subclasses give ``get_epoch_values(epoch)`` / ``get_update_values(num_updates)``"""

    def __init__(self, optimizer, param_group_field: str = "lr", noise_range_t=None, noise_type=None, noise_pct=None,
                 noise_std=None, noise_seed=None, initialize: bool = True) -> None:
        if any(a is not None for a in (noise_range_t, noise_type, noise_pct, noise_std, noise_seed)):
            raise NotImplementedError("mtlora_amd: LR noise is not implemented (the reference's build_scheduler never passes it); "
                                      "the noise arguments are accepted only as None")
        self.optimizer = optimizer
        self.param_group_field = param_group_field
        self._initial_param_group_field = f"initial_{param_group_field}"
        for i, group in enumerate(optimizer.param_groups):
            if initialize:
                if param_group_field not in group:
                    raise KeyError(f"{param_group_field} missing from param_groups[{i}]")
                group.setdefault(self._initial_param_group_field, group[param_group_field])
            elif self._initial_param_group_field not in group:
                raise KeyError(f"{self._initial_param_group_field} missing from param_groups[{i}]")
        self.base_values = [group[self._initial_param_group_field] for group in optimizer.param_groups]
        self.metric = None
        self.num_updates_seen = 0  # n + 1 after step_update(n): the number of optimizer updates made when it was called
        self.update_groups(self.base_values)

    def state_dict(self) -> Dict[str, Any]:
        return {key: value for key, value in self.__dict__.items() if key != "optimizer"}

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        self.__dict__.update(state_dict)

    def get_epoch_values(self, epoch: int):
        return None

    def get_update_values(self, num_updates: int):
        return None

    def step(self, epoch: int, metric: Optional[float] = None) -> None:
        self.metric = metric
        values = self.get_epoch_values(epoch)
        if values is not None:
            self.update_groups(values)

    def step_update(self, num_updates: int, metric: Optional[float] = None) -> None:
        self.metric = metric
        self.num_updates_seen = int(num_updates) + 1
        values = self.get_update_values(num_updates)
        if values is not None:
            self.update_groups(values)

    def update_groups(self, values) -> None:
        if not isinstance(values, (list, tuple)):
            values = [values] * len(self.optimizer.param_groups)
        for group, value in zip(self.optimizer.param_groups, values):
            group[self.param_group_field] = value


class _WarmupScheduler(Scheduler):
    """what the four schedules share: the linear warm-up from ``warmup_lr_init`` and the epoch / update switch"""

    def __init__(self, optimizer, warmup_t, warmup_lr_init, t_in_epochs, **base) -> None:
        super().__init__(optimizer, param_group_field="lr", **base)
        self.warmup_t = warmup_t
        self.warmup_lr_init = warmup_lr_init
        self.t_in_epochs = t_in_epochs
        if self.warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / self.warmup_t for v in self.base_values]
            super().update_groups(self.warmup_lr_init)
        else:
            self.warmup_steps = [1 for _ in self.base_values]

    def _warmup(self, t) -> List[float]:
        return [self.warmup_lr_init + t * s for s in self.warmup_steps]

    def _get_lr(self, t) -> List[float]:
        raise NotImplementedError

    def get_epoch_values(self, epoch: int):
        return self._get_lr(epoch) if self.t_in_epochs else None

    def get_update_values(self, num_updates: int):
        return self._get_lr(num_updates) if not self.t_in_epochs else None


class CosineLRScheduler(_WarmupScheduler):
    """timm 0.9.2's cosine schedule restricted to ONE cycle without decay (``cycle_mul = cycle_decay = k_decay = cycle_limit =
    1``, what the reference builds); any other value of those raises"""

    def __init__(self, optimizer, t_initial: int, lr_min: float = 0., cycle_mul: float = 1., cycle_decay: float = 1.,
                 cycle_limit: int = 1, warmup_t=0, warmup_lr_init=0, warmup_prefix=False, t_in_epochs=True, noise_range_t=None,
                 noise_pct=None, noise_std=None, noise_seed=None, k_decay=1.0, initialize=True) -> None:
        if cycle_mul != 1 or cycle_decay != 1 or k_decay != 1 or cycle_limit != 1:
            raise NotImplementedError("mtlora_amd: CosineLRScheduler implements cycle_mul = cycle_decay = k_decay = cycle_limit = 1 "
                                      f"only (got {cycle_mul}, {cycle_decay}, {k_decay}, {cycle_limit})")
        assert t_initial > 0 and lr_min >= 0
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, noise_range_t=noise_range_t, noise_pct=noise_pct,
                         noise_std=noise_std, noise_seed=noise_seed, initialize=initialize)
        self.t_initial = t_initial
        self.lr_min = lr_min
        self.cycle_mul, self.cycle_decay, self.cycle_limit, self.k_decay = cycle_mul, cycle_decay, cycle_limit, k_decay
        self.warmup_prefix = warmup_prefix

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self._warmup(t)
        if self.warmup_prefix:
            t = t - self.warmup_t
        i = t // self.t_initial
        t_curr = t - self.t_initial * i
        if i < self.cycle_limit:
            return [self.lr_min + 0.5 * (v - self.lr_min) * (1 + math.cos(math.pi * t_curr / self.t_initial)) for v in self.base_values]
        return [self.lr_min for _ in self.base_values]


class StepLRScheduler(_WarmupScheduler):
    """timm 0.9.2's step schedule: the base value times ``decay_rate`` every ``decay_t``"""

    def __init__(self, optimizer, decay_t: float, decay_rate: float = 1., warmup_t=0, warmup_lr_init=0, warmup_prefix=True,
                 t_in_epochs=True, noise_range_t=None, noise_pct=None, noise_std=None, noise_seed=None, initialize=True) -> None:
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, noise_range_t=noise_range_t, noise_pct=noise_pct,
                         noise_std=noise_std, noise_seed=noise_seed, initialize=initialize)
        self.decay_t = decay_t
        self.decay_rate = decay_rate
        self.warmup_prefix = warmup_prefix  # (kept for the signature: 0.9.2's step schedule does not read it)

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self._warmup(t)
        return [v * (self.decay_rate ** (t // self.decay_t)) for v in self.base_values]


class LinearLRScheduler(_WarmupScheduler):
    """the reference's own linear decay from the base value to ``lr_min_rate`` times it at ``t_initial``"""

    def __init__(self, optimizer, t_initial: int, lr_min_rate: float, warmup_t=0, warmup_lr_init=0., t_in_epochs=True,
                 noise_range_t=None, noise_pct=None, noise_std=None, noise_seed=None, initialize=True) -> None:
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, noise_range_t=noise_range_t, noise_pct=noise_pct,
                         noise_std=noise_std, noise_seed=noise_seed, initialize=initialize)
        self.t_initial = t_initial
        self.lr_min_rate = lr_min_rate

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self._warmup(t)
        t = t - self.warmup_t
        total_t = self.t_initial - self.warmup_t
        return [v - ((v - v * self.lr_min_rate) * (t / total_t)) for v in self.base_values]


class MultiStepLRScheduler(_WarmupScheduler):
    """the reference's own multi-step decay: the base value times ``gamma`` per milestone passed"""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_t=0, warmup_lr_init=0, t_in_epochs=True) -> None:
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs)
        self.milestones = milestones
        self.gamma = gamma
        assert self.warmup_t <= min(self.milestones)

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self._warmup(t)
        return [v * (self.gamma ** bisect.bisect_right(self.milestones, t)) for v in self.base_values]
