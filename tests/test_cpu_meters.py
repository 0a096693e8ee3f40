"""TrainMeters without a GPU: update_torch (the definition the kernel is held to) against a hand-written AverageMeter, the period,
the non-finite rule, reset, the construction errors, for_train_step's slot set, and what mtlora_meter_update rejects before any
launch."""
import math

import pytest
import torch

OK, SHAPE, NULL = 0, -2, -4
PASCAL4 = ("semseg", "normals", "sal", "human_parts")


class AverageMeter:
    """timm's (utils/metrics.py), as the reference's train loop uses it (main.py:318-321)"""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def bank_of(srcs, ns=None, periods=None):
    from mtlora_amd.meters import TrainMeters
    m = TrainMeters("cpu")
    for i, s in enumerate(srcs):
        m.add(f"m{i}", s, 1 if ns is None else ns[i], 1 if periods is None else periods[i])
    return m.seal()


def read(m):
    m.snapshot()
    return m.latest()


@pytest.mark.parametrize("n", [1, 3])
def test_update_torch_equals_average_meter(n):
    """50 steps of random fp32 losses: val, sum, count and avg EQUAL the AverageMeter's, which adds Python floats (fp64) one by one"""
    g = torch.Generator().manual_seed(5)
    losses = torch.rand(50, generator=g, dtype=torch.float32) * 7.0
    src = torch.zeros((), dtype=torch.float32)
    m, ref = bank_of([src], ns=[n]), AverageMeter()
    for k in range(50):
        src.copy_(losses[k])
        m.update_torch()
        ref.update(losses[k].item(), n)
        got = read(m)["m0"]
        assert (got.val, got.sum, got.count, got.avg, got.skipped) == (ref.val, ref.sum, ref.count, ref.avg, 0), k
    assert m.latest_calls == 50 and int(m.counter) == 50


def test_update_is_update_torch_on_a_cpu_bank_and_fp64_sources_are_taken():
    a, b = torch.tensor(0.1, dtype=torch.float64), torch.tensor([0.25], dtype=torch.float32)
    lr = torch.tensor([1e-3, 2e-3], dtype=torch.float64)
    m = bank_of([a, b, lr[1]])  # (a view of a larger tensor is fine)
    m.update()
    m.update()
    got = read(m)
    assert got["m0"].sum == 0.1 + 0.1 and got["m1"].avg == 0.25 and got["m2"].val == 2e-3 and got["m2"].count == 2


def test_period_three_changes_the_slot_at_calls_3_6_9_only():
    src = torch.zeros((), dtype=torch.float32)
    m = bank_of([src, src], periods=[3, 1])
    before = m.bank[0].clone()
    changed = []
    for call in range(1, 11):
        src.fill_(float(call))
        m.update_torch()
        if not torch.equal(m.bank[0], before):
            changed.append(call)
            before = m.bank[0].clone()
    assert changed == [3, 6, 9]
    got = read(m)
    assert (got["m0"].val, got["m0"].sum, got["m0"].count) == (9.0, 18.0, 3.0)
    assert (got["m1"].val, got["m1"].sum, got["m1"].count) == (10.0, 55.0, 10.0)


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan], ids=["inf", "neginf", "nan"])
def test_a_non_finite_value_is_counted_not_summed(bad):
    src = torch.zeros((), dtype=torch.float32)
    m = bank_of([src], ns=[2])
    for v in (1.5, 2.5):
        src.fill_(v)
        m.update_torch()
    src.fill_(bad)
    m.update_torch()
    got = read(m)["m0"]
    assert (got.sum, got.count, got.skipped, got.avg) == (8.0, 4.0, 1, 2.0)
    assert got.val == bad or (math.isnan(bad) and math.isnan(got.val))
    src.fill_(4.0)
    m.update_torch()
    got = read(m)["m0"]
    assert (got.val, got.sum, got.count, got.skipped) == (4.0, 16.0, 6.0, 1)


def test_reset_keeps_or_restarts_the_phase():
    src = torch.ones((), dtype=torch.float32)
    m = bank_of([src], periods=[3])
    for _ in range(4):
        m.update_torch()  # calls 1 .. 4: served at 3
    m.reset(keep_phase=True)
    assert int(m.counter) == 4 and not m.bank.any()
    m.update_torch()  # call 5
    assert read(m)["m0"].count == 0
    m.update_torch()  # call 6: served
    assert read(m)["m0"].count == 1
    m.reset(keep_phase=False)
    assert int(m.counter) == 0 and not m.bank.any()
    m.update_torch()
    m.update_torch()  # calls 1, 2 of the new phase
    assert read(m)["m0"].count == 0
    m.update_torch()
    assert read(m)["m0"].count == 1 and m.latest_calls == 3


def test_latest_is_empty_before_a_snapshot_and_avg_is_zero_without_a_count():
    m = bank_of([torch.ones((), dtype=torch.float32)], periods=[2])
    assert m.latest() == {} and m.latest(wait=True) == {}
    m.update()
    got = read(m)["m0"]
    assert (got.val, got.avg, got.sum, got.count, got.skipped) == (0.0, 0.0, 0.0, 0.0, 0)


def test_construction_errors():
    from mtlora_amd.meters import TrainMeters
    one = torch.zeros((), dtype=torch.float32)
    m = TrainMeters("cpu").add("a", one)
    with pytest.raises(TypeError):
        m.add("two", torch.zeros(2))
    with pytest.raises(TypeError):
        m.add("int", torch.zeros((), dtype=torch.int64))
    with pytest.raises(TypeError):
        m.add("half", torch.zeros((), dtype=torch.float16))
    with pytest.raises(TypeError):
        m.add("number", 1.0)
    with pytest.raises(ValueError):
        m.add("a", one)
    with pytest.raises(ValueError):
        m.add("p0", one, period=0)
    with pytest.raises(RuntimeError):
        m.update()  # not sealed
    m.seal()
    with pytest.raises(RuntimeError):
        m.add("late", one)
    full = TrainMeters("cpu")
    for i in range(64):
        full.add(f"s{i}", one)
    with pytest.raises(ValueError):
        full.add("s64", one)
    full.seal().update()
    assert len(read(full)) == 64


class _Opt:  # what for_train_step reads of an optimizer
    def __init__(self, sched):
        self.param_groups = [{"params": [torch.zeros(1)]}]
        self._sched = object() if sched else None
        self._lr = torch.tensor([5e-4, 5e-5], dtype=torch.float64)

    def lr_used(self):
        return self._lr


class _Scaler:  # ... and of a LossScaler
    def __init__(self):
        self._scale = None

    def _lazy_init(self, device):
        self._scale = torch.full((), 1024.0, dtype=torch.float32, device=device)


@pytest.mark.parametrize("with_scaler", [False, True], ids=["noscaler", "scaler"])
@pytest.mark.parametrize("with_sched", [False, True], ids=["nosched", "sched"])
def test_for_train_step_names_and_periods(with_scaler, with_sched):
    from mtlora_amd import meters as M
    scaler = _Scaler() if with_scaler else None
    m = M.for_train_step(PASCAL4, _Opt(with_sched), scaler, accumulation_steps=3)
    want = ["loss"] + [f"tasks/{t}/loss" for t in PASCAL4] + ["grad_norm"] + (["loss_scale"] if with_scaler else []) + \
        (["lr"] if with_sched else [])
    assert m.names == want
    assert dict(zip(m.names, m._period)) == {n: (3 if n == "grad_norm" else 1) for n in want}
    assert all(n == 1.0 for n in m._n)
    # the harness's call: three micro-steps, the norm with the third
    per = {t: torch.tensor(float(i + 1)) for i, t in enumerate(PASCAL4)}
    for call in range(3):
        m.stage_train_step(torch.tensor(10.0 + call), per, torch.tensor(0.5) if call == 2 else None)
    got = read(m)
    assert got["loss"].avg == 11.0 and got["loss"].count == 3 and got["tasks/sal/loss"].avg == 3.0
    assert (got["grad_norm"].val, got["grad_norm"].count) == (0.5, 1.0)
    if with_scaler:
        assert got["loss_scale"].val == 1024.0
    if with_sched:
        assert got["lr"].val == 5e-4
    with pytest.raises(ValueError):
        M.for_train_step(PASCAL4, _Opt(False), None, accumulation_steps=0)


def test_entry_points_reject_before_any_launch():
    """as test_cpu_attention_wide: validation comes first, so the calls are safe without a GPU -- 65 slots is a SHAPE error
    before any pointer is looked at, a null bank a NULL error"""
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    L = _lib.lib()
    assert _lib.METER_MAX_SLOTS == 64
    assert L.mtlora_meter_update(None, None, 65, None, None) == SHAPE
    assert L.mtlora_meter_update(None, None, 0, None, None) == SHAPE
    assert L.mtlora_meter_reset(None, 65, None, 1, None) == SHAPE
    assert L.mtlora_meter_update(None, None, 64, None, None) == NULL
    assert L.mtlora_meter_reset(None, 1, None, 0, None) == NULL
    import ctypes
    assert ctypes.sizeof(_lib.MeterSource) == 32 and _lib.MeterSource.weight.offset == 16 and _lib.MeterSource.period.offset == 24
