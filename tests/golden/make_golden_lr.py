#!/usr/bin/env python
"""Generate tests/golden/lr_schedules.json: the learning-rate tables tests/test_cpu_lr_scheduler.py holds mtlora_amd.lr_scheduler to.

    python tests/golden/make_golden_lr.py <directory of the reference checkout>

* ``linear`` and ``multistep`` are produced by the REFERENCE's own classes (its lr_scheduler.py, imported, not copied) over a stub
  ``timm.scheduler`` package: timm is not installed, and what the two classes take from it is the base class alone.  The stub
  base below is this project's restatement of the part of timm 0.9.2's ``Scheduler`` they use (``base_values`` from the groups'
  ``lr``, ``update_groups``).
* ``cosine``, ``cosine_prefix`` and ``step`` are timm 0.9.2's formulas (the requirements.txt pin) RESTATED here, since timm cannot
  be imported: one cycle, no cycle decay, k_decay = 1.
Only the json (data) is committed.  Floats are written with ``repr`` precision: they read back bit for bit.
"""
import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = [5e-4, 5e-5]
WARMUP_T, WARMUP_LR_INIT, T_INITIAL, LR_MIN, LR_MIN_RATE = 3, 1e-7, 12, 1e-6, 0.01
DECAY_T, DECAY_RATE, MILESTONES, GAMMA = 4, 0.5, [5, 9], 0.1
STEPS = 16


class _Optimizer:
    def __init__(self):
        self.param_groups = [{"lr": v} for v in BASE]


class _StubScheduler:
    def __init__(self, optimizer, param_group_field, **unused):
        self.optimizer, self.param_group_field = optimizer, param_group_field
        self.base_values = [g[param_group_field] for g in optimizer.param_groups]
        self.update_groups(self.base_values)

    def update_groups(self, values):
        if not isinstance(values, (list, tuple)):
            values = [values] * len(self.optimizer.param_groups)
        for g, v in zip(self.optimizer.param_groups, values):
            g[self.param_group_field] = v


def _import_reference(ref):
    mods = {n: types.ModuleType(n) for n in ("timm", "timm.scheduler", "timm.scheduler.cosine_lr", "timm.scheduler.step_lr",
                                             "timm.scheduler.scheduler")}
    mods["timm.scheduler.cosine_lr"].CosineLRScheduler = None  # (imported by name, not used by the two classes taken here)
    mods["timm.scheduler.step_lr"].StepLRScheduler = None
    mods["timm.scheduler.scheduler"].Scheduler = _StubScheduler
    sys.modules.update(mods)
    sys.path.insert(0, ref)
    import lr_scheduler
    return lr_scheduler


def _warmup(t, v):
    return WARMUP_LR_INIT + t * ((v - WARMUP_LR_INIT) / WARMUP_T)


def _cosine(t, v, prefix):  # timm 0.9.2 cosine_lr.py, restated
    if t < WARMUP_T:
        return _warmup(t, v)
    if prefix:
        t = t - WARMUP_T
    i = t // T_INITIAL
    t_curr = t - T_INITIAL * i
    return LR_MIN + 0.5 * (v - LR_MIN) * (1 + math.cos(math.pi * t_curr / T_INITIAL)) if i < 1 else LR_MIN


def _step(t, v):  # timm 0.9.2 step_lr.py, restated
    return _warmup(t, v) if t < WARMUP_T else v * (DECAY_RATE ** (t // DECAY_T))


def main():
    ref = sys.argv[1]
    R = _import_reference(ref)
    lin = R.LinearLRScheduler(_Optimizer(), t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE, warmup_t=WARMUP_T,
                              warmup_lr_init=WARMUP_LR_INIT, t_in_epochs=False)
    ms = R.MultiStepLRScheduler(_Optimizer(), milestones=MILESTONES, gamma=GAMMA, warmup_t=WARMUP_T, warmup_lr_init=WARMUP_LR_INIT,
                                t_in_epochs=False)
    out = {
        "settings": dict(base=BASE, warmup_t=WARMUP_T, warmup_lr_init=WARMUP_LR_INIT, t_initial=T_INITIAL, lr_min=LR_MIN,
                         lr_min_rate=LR_MIN_RATE, decay_t=DECAY_T, decay_rate=DECAY_RATE, milestones=MILESTONES, gamma=GAMMA),
        "source": {"linear": "reference classes", "multistep": "reference classes", "cosine": "restated from timm 0.9.2",
                   "cosine_prefix": "restated from timm 0.9.2", "step": "restated from timm 0.9.2"},
        "after_construction": {"linear": [g["lr"] for g in lin.optimizer.param_groups],
                               "multistep": [g["lr"] for g in ms.optimizer.param_groups]},
        "tables": {
            "linear": [lin.get_update_values(t) for t in range(STEPS)],
            "multistep": [ms.get_update_values(t) for t in range(STEPS)],
            "cosine": [[_cosine(t, v, False) for v in BASE] for t in range(STEPS)],
            "cosine_prefix": [[_cosine(t, v, True) for v in BASE] for t in range(STEPS)],
            "step": [[_step(t, v) for v in BASE] for t in range(STEPS)],
        },
    }
    with open(os.path.join(HERE, "lr_schedules.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
