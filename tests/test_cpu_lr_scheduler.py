"""Host side of the learning-rate schedules: mtlora_amd.lr_scheduler (the reference's lr_scheduler.py without timm) against closed
forms and the recorded tables of tests/golden/lr_schedules.json (linear / multistep from the reference's own classes, cosine / step
restated from timm 0.9.2 -- tests/golden/make_golden_lr.py), the additive exports of the device-side schedule and their bindings,
and what is rejected before any launch.  Pure host calls: no GPU.

The settings are the issue's: two param groups (5e-4, 5e-5), warmup_t 3, warmup_lr_init 1e-7, t_initial 12, lr_min 1e-6,
decay_t 4, decay_rate 0.5, milestones (5, 9), gamma 0.1, t = 0 .. 15; every value comparison is ``==`` on Python floats.
"""
import bisect
import ctypes
import inspect
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = [5e-4, 5e-5]
WARMUP_T, WARMUP_LR_INIT, T_INITIAL, LR_MIN, LR_MIN_RATE = 3, 1e-7, 12, 1e-6, 0.01
DECAY_T, DECAY_RATE, MILESTONES, GAMMA = 4, 0.5, [5, 9], 0.1
KINDS = ["cosine", "cosine_prefix", "step", "linear", "multistep"]


class AttrDict(dict):
    __getattr__ = dict.__getitem__


class FakeOptimizer:
    """what a Scheduler touches of an optimizer"""

    def __init__(self):
        self.param_groups = [{"lr": v, "params": []} for v in BASE]


def build(kind, optimizer=None):
    from mtlora_amd import lr_scheduler as S
    o = optimizer or FakeOptimizer()
    common = dict(warmup_t=WARMUP_T, warmup_lr_init=WARMUP_LR_INIT, t_in_epochs=False)
    if kind in ("cosine", "cosine_prefix"):
        return S.CosineLRScheduler(o, t_initial=T_INITIAL, lr_min=LR_MIN, warmup_prefix=(kind == "cosine_prefix"), **common)
    if kind == "step":
        return S.StepLRScheduler(o, decay_t=DECAY_T, decay_rate=DECAY_RATE, **common)
    if kind == "linear":
        return S.LinearLRScheduler(o, t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE, **common)
    return S.MultiStepLRScheduler(o, milestones=list(MILESTONES), gamma=GAMMA, **common)


def closed_form(kind, t, v):
    """the issue's formulas, in its expression order (the warm-up slope is formed first, as the reference's classes form it)"""
    if t < WARMUP_T:
        return WARMUP_LR_INIT + t * ((v - WARMUP_LR_INIT) / WARMUP_T)
    if kind in ("cosine", "cosine_prefix"):
        if kind == "cosine_prefix":
            t -= WARMUP_T
        i = t // T_INITIAL
        t_curr = t - T_INITIAL * i
        return LR_MIN + 0.5 * (v - LR_MIN) * (1 + math.cos(math.pi * t_curr / T_INITIAL)) if i < 1 else LR_MIN
    if kind == "step":
        return v * DECAY_RATE ** (t // DECAY_T)
    if kind == "linear":
        t -= WARMUP_T
        total = T_INITIAL - WARMUP_T
        return v - (v - v * LR_MIN_RATE) * (t / total)
    return v * GAMMA ** bisect.bisect_right(MILESTONES, t)


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "lr_schedules.json")) as f:
        return json.load(f)


def _header():
    return open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()


@pytest.mark.parametrize("kind", KINDS)
def test_values_equal_the_closed_forms_and_the_recorded_tables(kind):
    s = build(kind)
    table = golden()["tables"][kind]
    assert len(table) == 16
    for t in range(16):
        got = s._get_lr(t)
        assert got == [closed_form(kind, t, v) for v in BASE], (kind, t)
        assert got == table[t], (kind, t)
        assert s.get_update_values(t) == got and s.get_epoch_values(t) is None
    # the shapes the tables must have: warm-up starts at warmup_lr_init, the plateau / the decays are reached
    assert s._get_lr(0) == [WARMUP_LR_INIT] * 2
    if kind == "cosine":
        assert s._get_lr(12) == [LR_MIN] * 2 and s._get_lr(15) == [LR_MIN] * 2
    if kind == "cosine_prefix":
        assert s._get_lr(3) == BASE and s._get_lr(15) == [LR_MIN] * 2
    if kind == "step":
        assert s._get_lr(8) == [v * 0.25 for v in BASE]
    if kind == "linear":
        assert s._get_lr(3) == BASE and s._get_lr(12) == [v - (v - v * LR_MIN_RATE) * 1.0 for v in BASE]
    if kind == "multistep":
        assert s._get_lr(4) == BASE and s._get_lr(5) == [v * 0.1 for v in BASE] and s._get_lr(9) == [v * 0.1 ** 2 for v in BASE]


def test_recorded_tables_say_where_they_come_from():
    g = golden()
    assert g["source"]["linear"] == g["source"]["multistep"] == "reference classes"
    assert all(g["source"][k] == "restated from timm 0.9.2" for k in ("cosine", "cosine_prefix", "step"))
    assert g["after_construction"] == {"linear": [WARMUP_LR_INIT] * 2, "multistep": [WARMUP_LR_INIT] * 2}
    assert g["settings"]["base"] == BASE and g["settings"]["milestones"] == MILESTONES


@pytest.mark.parametrize("kind", KINDS)
def test_groups_step_update_and_state_dict(kind):
    o = FakeOptimizer()
    s = build(kind, o)
    assert [g["lr"] for g in o.param_groups] == [WARMUP_LR_INIT] * 2  # the constructor's value is _get_lr(0)
    assert [g["initial_lr"] for g in o.param_groups] == BASE and s.base_values == BASE
    assert s.num_updates_seen == 0
    s.step_update(7)
    assert [g["lr"] for g in o.param_groups] == s._get_lr(7) and s.num_updates_seen == 8
    s.step(2)  # counted in updates: an epoch step writes nothing
    assert [g["lr"] for g in o.param_groups] == s._get_lr(7)
    sd = s.state_dict()
    assert "optimizer" not in sd and sd["warmup_t"] == WARMUP_T and sd["base_values"] == BASE
    fresh = build(kind)
    fresh.warmup_t = 99
    fresh.load_state_dict(sd)
    assert fresh.state_dict() == sd and fresh.num_updates_seen == 8
    assert [fresh._get_lr(t) for t in range(16)] == [s._get_lr(t) for t in range(16)]
    # in epochs, the host classes step by epoch
    from mtlora_amd import lr_scheduler as S
    e = S.LinearLRScheduler(FakeOptimizer(), t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE, warmup_t=WARMUP_T,
                            warmup_lr_init=WARMUP_LR_INIT, t_in_epochs=True)
    e.step(5)
    assert [g["lr"] for g in e.optimizer.param_groups] == e._get_lr(5) and e.get_update_values(5) is None


def test_no_warmup_leaves_the_groups_at_their_base_values():
    from mtlora_amd import lr_scheduler as S
    o = FakeOptimizer()
    s = S.StepLRScheduler(o, decay_t=DECAY_T, decay_rate=DECAY_RATE, t_in_epochs=False)
    assert [g["lr"] for g in o.param_groups] == BASE and s._get_lr(0) == BASE


def config(name, prefix=False):
    return AttrDict(TRAIN=AttrDict(EPOCHS=4, WARMUP_EPOCHS=1, MIN_LR=LR_MIN, WARMUP_LR=WARMUP_LR_INIT,
                                   LR_SCHEDULER=AttrDict(NAME=name, WARMUP_PREFIX=prefix, DECAY_EPOCHS=2, DECAY_RATE=DECAY_RATE,
                                                         MULTISTEPS=[2, 3], GAMMA=GAMMA)))


def test_build_scheduler():
    from mtlora_amd import lr_scheduler as S
    n = 5  # iterations per epoch: 20 steps, 5 of warm-up
    c = S.build_scheduler(config("cosine"), FakeOptimizer(), n)
    assert type(c) is S.CosineLRScheduler and (c.t_initial, c.warmup_t, c.lr_min, c.warmup_prefix, c.cycle_limit) == (20, 5, LR_MIN, False, 1)
    c = S.build_scheduler(config("cosine", prefix=True), FakeOptimizer(), n)
    assert (c.t_initial, c.warmup_t, c.warmup_prefix) == (15, 5, True)
    l = S.build_scheduler(config("linear"), FakeOptimizer(), n)
    assert type(l) is S.LinearLRScheduler and (l.t_initial, l.warmup_t, l.lr_min_rate) == (20, 5, 0.01)
    s = S.build_scheduler(config("step"), FakeOptimizer(), n)
    assert type(s) is S.StepLRScheduler and (s.decay_t, s.decay_rate, s.warmup_t) == (10, DECAY_RATE, 5)
    m = S.build_scheduler(config("multistep"), FakeOptimizer(), n)
    assert type(m) is S.MultiStepLRScheduler and (m.milestones, m.gamma, m.warmup_t) == ([10, 15], GAMMA, 5)
    for x in (c, l, s, m):
        assert x.t_in_epochs is False and x.warmup_lr_init == WARMUP_LR_INIT
        assert [g["lr"] for g in x.optimizer.param_groups] == [WARMUP_LR_INIT] * 2
    assert S.build_scheduler(config("plateau"), FakeOptimizer(), n) is None


def test_what_the_host_classes_refuse():
    from mtlora_amd import lr_scheduler as S
    for noise in (dict(noise_range_t=5), dict(noise_pct=0.67), dict(noise_std=1.0), dict(noise_seed=42)):
        with pytest.raises(NotImplementedError, match="noise"):
            S.LinearLRScheduler(FakeOptimizer(), t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE, **noise)
        with pytest.raises(NotImplementedError, match="noise"):
            S.CosineLRScheduler(FakeOptimizer(), t_initial=T_INITIAL, **noise)
    for bad in (dict(cycle_mul=2.0), dict(cycle_decay=0.5), dict(k_decay=0.5), dict(cycle_limit=2)):
        with pytest.raises(NotImplementedError, match="cycle"):
            S.CosineLRScheduler(FakeOptimizer(), t_initial=T_INITIAL, **bad)
    with pytest.raises(AssertionError):  # the reference's assertion: the warm-up ends in front of the first milestone
        S.MultiStepLRScheduler(FakeOptimizer(), milestones=[2, 9], warmup_t=3)


# ---- the device-side schedule: exports, bindings, pure host rejects -----------------------------------------------------------
def test_schedule_exports_are_declared_and_bound():
    from mtlora_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    for name in ("mtlora_adamw_sched_update_dev", "mtlora_lr_schedule_check", "mtlora_lr_schedule_value"):
        assert name in protos and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
        assert len(protos[name].split(",")) == len(_lib._SIGS[name][1]), name
    params = [" ".join(p.split()) for p in protos["mtlora_adamw_sched_update_dev"].split(",")]
    accum = [" ".join(p.split()) for p in protos["mtlora_adamw_accum_update_dev"].split(",")]
    res, argtypes = _lib._SIGS["mtlora_adamw_sched_update_dev"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == 21
    # mtlora_adamw_accum_update_dev's parameters, then the schedule buffer, then the stream
    assert params[:19] == accum[:19] and params[19:] == ["void* sched_dev", "void* stream"]
    assert argtypes[:19] == _lib._SIGS["mtlora_adamw_accum_update_dev"][1][:19]
    h = _header()
    assert "#define MTLORA_ABI_VERSION 12" in h and _lib.ABI_VERSION == 12 == _lib.lib().mtlora_version()
    assert "#define MTLORA_ADAMW_CTRL_WORDS 64" in h and _lib.ADAMW_CTRL_WORDS == 64
    assert "#define MTLORA_ADAMW_GROUPS_DEV_BYTES 1152" in h and _lib.ADAMW_GROUPS_DEV_BYTES == 1152
    assert f"#define MTLORA_LR_MAX_MILESTONES {_lib.LR_MAX_MILESTONES}" in h and _lib.LR_MAX_MILESTONES == 16
    for name, value in (("COSINE", _lib.LR_COSINE), ("STEP", _lib.LR_STEP), ("LINEAR", _lib.LR_LINEAR), ("MULTISTEP", _lib.LR_MULTISTEP)):
        assert f"#define MTLORA_LR_{name} {value}\n" in h
    assert f"#define MTLORA_ADAMW_SCHED_DEV_BYTES {_lib.ADAMW_SCHED_DEV_BYTES}\n" in h
    assert f"#define MTLORA_ADAMW_SCHED_COUNT_OFFSET {_lib.ADAMW_SCHED_COUNT_OFFSET} " in h
    assert f"#define MTLORA_ADAMW_SCHED_LR_OFFSET {_lib.ADAMW_SCHED_LR_OFFSET}\n" in h
    # the record is the buffer's head; the count and lr_used[MAX_GROUPS] follow it
    assert ctypes.sizeof(_lib.LrSchedule) == _lib.ADAMW_SCHED_COUNT_OFFSET == _lib.ADAMW_SCHED_LR_OFFSET - 8
    assert _lib.ADAMW_SCHED_DEV_BYTES == _lib.ADAMW_SCHED_LR_OFFSET + 8 * _lib.ADAMW_MAX_GROUPS
    assert _lib.LrSchedule.milestones.size == 8 * _lib.LR_MAX_MILESTONES and _lib.LrSchedule.base_lr.size == 8 * _lib.ADAMW_MAX_GROUPS


def bare_optimizer(capturable=True):
    """a FusedAdamW with only what the host-side checks read: nothing touches a device"""
    from mtlora_amd.optim import FusedAdamW
    opt = FusedAdamW.__new__(FusedAdamW)
    opt._capturable = capturable
    opt.param_groups = FakeOptimizer().param_groups
    return opt


@pytest.mark.parametrize("kind", KINDS)
def test_the_record_evaluates_to_the_host_values(kind):
    """the function the kernel runs, compiled for the host (mtlora_lr_schedule_value): the record FusedAdamW fills from the
    scheduler gives the scheduler's values.  Bit for bit where only + - * / are involved (warm-up, linear, the lr_min plateau);
    within a relative 2^-40 where the C library's cos / pow come in (they are CPython's own here, but that is not relied on)."""
    from mtlora_amd import _lib
    s = build(kind)
    rec = bare_optimizer()._schedule_record(s)
    assert rec.kind == {"cosine": 1, "cosine_prefix": 1, "step": 2, "linear": 3, "multistep": 4}[kind]
    for t in list(range(16)) + [2 ** 24 + 1, 2 ** 40]:
        want = s._get_lr(t)
        for g in range(2):
            out = ctypes.c_double()
            assert _lib.lib().mtlora_lr_schedule_value(ctypes.byref(rec), 2, g, t, ctypes.byref(out)) == 0
            exact = t < WARMUP_T or kind == "linear" or want[g] == LR_MIN
            if exact:
                assert out.value == want[g], (kind, t, g)
            else:
                assert abs(out.value - want[g]) <= 2.0 ** -40 * abs(want[g]), (kind, t, g)
    out = ctypes.c_double()
    assert _lib.lib().mtlora_lr_schedule_value(ctypes.byref(rec), 2, 2, 0, ctypes.byref(out)) == -2  # group out of range
    assert _lib.lib().mtlora_lr_schedule_value(ctypes.byref(rec), 2, 0, -1, ctypes.byref(out)) == -2
    assert _lib.lib().mtlora_lr_schedule_value(ctypes.byref(rec), 2, 0, 0, None) == -4


def test_invalid_records_are_rejected_on_the_host():
    """mtlora_lr_schedule_check is the kernel's own validation: MTLORA_ERR_SHAPE (-2) for what the device would answer with
    found_inf"""
    from mtlora_amd import _lib
    L = _lib.lib()

    def check(which, **fields):
        rec = bare_optimizer()._schedule_record(build(which))
        for k, v in fields.items():
            if k == "milestones":
                for i, m in enumerate(v):
                    rec.milestones[i] = m
            elif k == "base0":
                rec.base_lr[0] = v
            else:
                setattr(rec, k, v)
        return L.mtlora_lr_schedule_check(ctypes.byref(rec), 2)

    nan = float("nan")
    for kind in KINDS:
        assert check(kind) == 0
        assert check(kind, kind=0) == -2 and check(kind, kind=5) == -2
        assert check(kind, warmup_t=-1) == -2 and check(kind, warmup_lr_init=nan) == -2 and check(kind, warmup_lr_init=-1e-3) == -2
        assert check(kind, base0=nan) == -2 and check(kind, base0=-1.0) == -2
    assert check("cosine", lr_min=nan) == -2 and check("cosine", lr_min=-1e-6) == -2 and check("cosine", t_initial=0) == -2
    assert check("linear", t_initial=WARMUP_T) == -2 and check("linear", lr_min_rate=nan) == -2
    assert check("step", decay_t=0) == -2 and check("step", decay_rate=nan) == -2
    assert check("multistep", gamma=nan) == -2
    assert check("multistep", n_milestones=_lib.LR_MAX_MILESTONES + 1) == -2 and check("multistep", n_milestones=-1) == -2
    assert check("multistep", milestones=[9, 5]) == -2  # not ascending
    assert check("multistep", milestones=[2, 9]) == -2  # inside the warm-up
    assert check("multistep", warmup_t=0, milestones=[0, 9]) == -2  # milestones >= 1: _get_lr(0) is the constructor's value
    assert check("multistep", n_milestones=0) == 0
    rec = _lib.LrSchedule()
    assert L.mtlora_lr_schedule_check(None, 2) == -4
    assert L.mtlora_lr_schedule_check(ctypes.byref(rec), 0) == -7 and L.mtlora_lr_schedule_check(ctypes.byref(rec), 17) == -7
    assert L.mtlora_lr_schedule_check(ctypes.byref(rec), 2) == -2  # an all-zero record: unknown kind


def test_sched_update_rejects_before_any_launch():
    """null pointers -> MTLORA_ERR_NULL (-4), the schedule buffer among them; accum_steps out of range -> MTLORA_ERR_SHAPE (-2);
    misaligned buffers -> MTLORA_ERR_ALIGN (-3).  With accum_steps == 1 acc and acc_offsets may be null: that call passes every
    check, so it is NOT made here (it would launch).  No device is touched."""
    from mtlora_amd import _lib
    L = _lib.lib()

    def call(table=16, grads=16, groups=16, n_groups=1, ctrl=16, scratch=16, scratch_bytes=8, acc=16, acc_offsets=16, k=2, sched=16):
        return L.mtlora_adamw_sched_update_dev(table, grads, 1, 1, groups, n_groups, 0.0, ctrl, None, None, None, 2.0, 0.5, 1, scratch,
                                               scratch_bytes, acc, acc_offsets, k, sched, None)

    for name in ("table", "grads", "groups", "ctrl", "scratch", "acc", "acc_offsets", "sched"):
        assert call(**{name: None}) == -4, name
    assert call(k=1, sched=None) == -4 and call(k=1, acc=None, acc_offsets=None, sched=None) == -4
    for k in (0, -1, _lib.ADAMW_MAX_ACCUM_STEPS + 1):
        assert call(k=k) == -2, k
    assert call(n_groups=0) == -7 and call(n_groups=_lib.ADAMW_MAX_GROUPS + 1) == -7
    assert call(n_groups=_lib.ADAMW_MAX_GROUPS, scratch_bytes=4) == -5
    assert call(sched=20) == -3 and call(groups=20) == -3 and call(acc=20) == -3 and call(acc_offsets=20) == -3
    assert call(k=1, acc=None, acc_offsets=None, sched=20) == -3


def test_attach_schedule_argument_checks():
    """a by-value optimizer -> TypeError; something that is no scheduler of this package -> TypeError; a scheduler counted in
    epochs, too many milestones, a group count that does not match -> ValueError; all before a device is touched"""
    from mtlora_amd import _lib
    from mtlora_amd import lr_scheduler as S
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW
    p = inspect.signature(FusedAdamW.attach_schedule).parameters
    assert list(p)[1:] == ["scheduler", "num_updates"] and p["num_updates"].default is None
    for name in ("detach_schedule", "lr_used", "num_updates"):
        assert callable(getattr(FusedAdamW, name))
    with pytest.raises(TypeError, match="capturable=True"):
        bare_optimizer(capturable=False).attach_schedule(build("linear"))
    opt = bare_optimizer()
    with pytest.raises(TypeError, match="lr_scheduler"):
        opt._schedule_record(object())
    with pytest.raises(ValueError, match="t_in_epochs"):
        opt._schedule_record(S.LinearLRScheduler(FakeOptimizer(), t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE))
    many = list(range(5, 5 + _lib.LR_MAX_MILESTONES + 1))
    with pytest.raises(ValueError, match="milestones"):
        opt._schedule_record(S.MultiStepLRScheduler(FakeOptimizer(), milestones=many, warmup_t=WARMUP_T, t_in_epochs=False))
    assert opt._schedule_record(S.MultiStepLRScheduler(FakeOptimizer(), milestones=many[:-1], warmup_t=WARMUP_T,
                                                       t_in_epochs=False)).n_milestones == _lib.LR_MAX_MILESTONES
    opt.param_groups = opt.param_groups[:1]
    with pytest.raises(ValueError, match="groups"):
        opt._schedule_record(build("linear"))
    bad = build("cosine")
    bad.lr_min = float("nan")
    with pytest.raises(ValueError, match="cannot run on the device"):
        bare_optimizer()._schedule_record(bad)
    # GraphedTrainStep: a torch optimizer cannot take the schedule into its update
    import torch
    assert inspect.signature(H.GraphedTrainStep.__init__).parameters["lr_scheduler"].default is None
    sgd = torch.optim.SGD(torch.nn.Linear(2, 2).parameters(), lr=0.1)
    with pytest.raises(TypeError, match="lr_scheduler"):
        H.GraphedTrainStep(None, None, sgd, torch.zeros(1), {}, lr_scheduler=build("linear"))
