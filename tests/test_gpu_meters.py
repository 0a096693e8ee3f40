"""TrainMeters on the GPU: the update kernel (csrc/meter.hip) against its definition (TrainMeters.update_torch on a CPU copy of the
same sources, bit for bit), the meters inside train_step and inside the captured GraphedTrainStep (they count what the step
returns and change nothing it computes), the read-back that never synchronises, and a non-finite step under the fp16 recipe."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = ["semseg", "normals", "sal", "human_parts"]
MODEL_KW = dict(img_size=224, tasks=TASKS, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4)  # test_gpu_lr_schedule's
INIT_SCALE = 2.0 ** 10


def dev():
    return torch.device("cuda:0")


# ---- 1. the kernel against the definition ---------------------------------------------------------------------------------------
def _pair(dtypes, ns, periods):
    """the same bank twice: GPU sources under the kernel, CPU sources under update_torch"""
    from mtlora_amd.meters import TrainMeters
    banks, srcs = [], []
    for d in (dev(), torch.device("cpu")):
        s = [torch.zeros((), dtype=dt, device=d) for dt in dtypes]
        m = TrainMeters(d)
        for i, t in enumerate(s):
            m.add(f"m{i}", t, ns[i], periods[i])
        banks.append(m.seal())
        srcs.append(s)
    return banks, srcs


def _run_pair(dtypes, ns, periods, calls, inject):
    (gpu, cpu), (gs, cs) = _pair(dtypes, ns, periods)
    g = torch.Generator().manual_seed(11)
    for call in range(1, calls + 1):
        vals = torch.rand(len(dtypes), generator=g, dtype=torch.float64) * 9.0 - 1.0
        for i in range(len(dtypes)):
            v = inject.get((i, call), vals[i].item())
            gs[i].fill_(v)
            cs[i].fill_(v)
        gpu.update()
        cpu.update_torch()
    torch.cuda.synchronize()
    # int64 words (bank, then the counter): equal bit patterns, so a nan val compares as well
    assert torch.equal(gpu._state.cpu(), cpu._state), (gpu.bank.cpu(), cpu.bank)
    assert int(gpu.counter) == calls
    return gpu, cpu


def test_kernel_equals_definition():
    f32, f64 = torch.float32, torch.float64
    gpu, cpu = _run_pair([f32, f32, f64, f32, f64], [1, 2, 1, 2, 1], [1, 1, 2, 3, 1], 12, {(1, 4): math.inf, (3, 6): math.nan})
    b = cpu.bank
    assert b[1, 3] == 1 and b[3, 3] == 1 and b[:, 3].sum() == 2      # the two injected values were seen and left out
    assert b[:, 2].tolist() == [12.0, 22.0, 6.0, 6.0, 12.0]           # counts: n x served calls (4 served of slot 3, one skipped)
    assert math.isnan(b[3, 0].item()) is False and torch.isfinite(b[:, 1]).all()  # later values replaced val; no sum was poisoned
    gpu.snapshot()
    got = gpu.latest(wait=True)
    assert got["m1"].skipped == 1 and got["m1"].count == 22.0 and got["m1"].avg == b[1, 1].item() / 22.0 and gpu.latest_calls == 12


def test_kernel_last_lane_and_single_lane():
    f32, f64 = torch.float32, torch.float64
    _run_pair([f32 if i % 3 else f64 for i in range(64)], [1 + i % 2 for i in range(64)], [1 + i % 4 for i in range(64)], 9,
              {(63, 8): math.inf, (0, 3): math.nan})
    _run_pair([f32], [1], [2], 5, {(0, 4): -math.inf})


def test_reset_kernel_keeps_or_restarts_the_phase():
    (gpu, _), (gs, _) = _pair([torch.float32] * 3, [1, 1, 1], [1, 2, 3])
    for t in gs:
        t.fill_(2.0)
    for _ in range(3):
        gpu.update()
    gpu.reset(keep_phase=True)
    torch.cuda.synchronize()
    assert int(gpu.counter) == 3 and not gpu.bank.any()
    gpu.update()  # call 4: slots 0 and 1
    assert gpu.bank[:, 2].tolist() == [1.0, 1.0, 0.0]
    gpu.reset(keep_phase=False)
    assert int(gpu.counter) == 0 and not gpu.bank.any()


# ---- 2. / 3. / 5. inside the train step -------------------------------------------------------------------------------------------
def _setup(capturable):
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import LossScaler
    torch.manual_seed(9)
    Fn._seed_counter = 0
    img, tg = H.synthetic_batch(2, 224, TASKS, seed=17, device=dev())
    model = H.build_model(**MODEL_KW).to(dev()).train()
    opt = H.build_optimizer(model, lr=5e-4, impl="hip", capturable=capturable)
    return H, model, opt, LossScaler(init_scale=INIT_SCALE), img, tg


def _running_mean(values):
    s = 0.0
    for v in values:  # sequential fp64 adds, as AverageMeter's
        s += v
    return s / len(values)


def test_eager_step_with_meters():
    from mtlora_amd.meters import TrainMeters
    runs = {}
    for with_meters in (True, False):
        H, model, opt, scaler, img, tg = _setup(capturable=False)

        class Recording(H.MultiTaskLoss):  # the per-task losses as the step computed them
            seen = []

            def combine(self, per):
                self.seen.append({t: per[t].detach().clone() for t in TASKS})
                return super().combine(per)

        crit = Recording(TASKS)
        crit.seen = []
        meters = TrainMeters.for_train_step(TASKS, opt, scaler) if with_meters else None
        losses = []
        for _ in range(6):
            kw = dict(meters=meters) if with_meters else {}
            loss, norm = H.train_step(model, crit, opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler, **kw)
            losses.append(loss.clone())
        torch.cuda.synchronize()
        runs[with_meters] = (losses, [p.detach().clone() for p in model.parameters()], crit.seen, meters, scaler, norm)
    (la, pa, seen, meters, scaler, norm), (lb, pb, _, _, _, _) = runs[True], runs[False]
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and all(torch.isfinite(a).all() for a in la)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert meters.names == ["loss"] + [f"tasks/{t}/loss" for t in TASKS] + ["grad_norm", "loss_scale"]
    meters.snapshot()
    got = meters.latest(wait=True)
    assert meters.latest_calls == 6
    assert got["loss"].count == 6 and got["loss"].skipped == 0
    assert got["loss"].avg == _running_mean([l.item() for l in la]) and got["loss"].val == la[-1].item()
    for t in TASKS:
        m = got[f"tasks/{t}/loss"]
        assert m.count == 6 and m.avg == _running_mean([s[t].item() for s in seen]), t
    assert got["grad_norm"].count + got["grad_norm"].skipped == 6 and got["grad_norm"].val == norm.item()
    assert got["loss_scale"].val == scaler.get_scale()


def _graphed(with_meters, k, with_sched):
    from mtlora_amd import lr_scheduler as S
    from mtlora_amd.meters import TrainMeters
    H, model, opt, scaler, img, tg = _setup(capturable=True)
    sched = None
    if with_sched:
        sched = S.LinearLRScheduler(opt, t_initial=12, lr_min_rate=0.01, warmup_t=3, warmup_lr_init=1e-7, t_in_epochs=False)
        opt.attach_schedule(sched)  # before the meters are built: they bind lr_used()
    meters = TrainMeters.for_train_step(TASKS, opt, scaler, accumulation_steps=k) if with_meters else None
    kw = dict(meters=meters) if with_meters else {}
    gs = H.GraphedTrainStep(model, H.MultiTaskLoss(TASKS), opt, img, tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16,
                            loss_scaler=scaler, accumulation_steps=k, lr_scheduler=sched, **kw)
    assert gs.graphed is True and gs.why == "", gs.why
    return gs, model, opt, scaler, img, meters


def test_graphed_step_with_meters():
    from mtlora_amd import functional as Fn
    try:
        gs, model, opt, scaler, _, meters = _graphed(True, 2, True)
        assert "lr" in meters.names and int(meters.counter) == 0 and not meters.bank.any()  # the warm-up did not leak in
        losses = []
        for _ in range(8):
            losses.append(gs().clone())
        meters.snapshot()
        got = meters.latest(wait=True)
        torch.cuda.synchronize()
        assert meters.latest_calls == 8 == gs._calls
        assert got["loss"].count == 8 and got["grad_norm"].count == 4
        assert got["grad_norm"].val == gs.grad_norm.item()
        assert got["lr"].val == opt.lr_used()[0].item() and got["lr"].val > 0.0
        assert got["loss_scale"].val == scaler.get_scale()
        assert got["loss"].avg == _running_mean([l.item() for l in losses]) and got["loss"].skipped == 0
        params = [p.detach().clone() for p in model.parameters()]
        gs2, model2, _, _, _, _ = _graphed(False, 2, True)
        for i in range(8):
            assert torch.equal(gs2(), losses[i]), i
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(params, model2.parameters()))
    finally:
        Fn.set_seed_offset(None)


def test_graphed_non_finite_step():
    from mtlora_amd import functional as Fn
    try:
        gs, model, opt, scaler, img, meters = _graphed(True, 1, False)
        good = img.clone()
        gs()
        gs()
        img.fill_(1e30)  # overflows the fp16 forward: the loss is inf or nan
        bad = gs().clone()
        img.copy_(good)
        meters.snapshot()
        got = meters.latest(wait=True)
        assert not torch.isfinite(bad).all()
        assert got["loss"].skipped == 1 and got["loss"].count == 2 and not math.isfinite(got["loss"].val)
        assert math.isfinite(got["loss"].avg) and math.isfinite(got["loss"].sum)
        assert got["loss_scale"].val == INIT_SCALE * 0.5 == scaler.get_scale()  # the scaler backed off
        after = gs().clone()
        meters.snapshot()
        got = meters.latest(wait=True)
        assert torch.isfinite(after).all()
        assert got["loss"].skipped == 1 and got["loss"].count == 3 and got["loss"].val == after.item()
        assert got["grad_norm"].count + got["grad_norm"].skipped == 4 and math.isfinite(got["grad_norm"].val)
    finally:
        Fn.set_seed_offset(None)


# ---- 4. reading back never stalls -------------------------------------------------------------------------------------------------
def test_snapshot_and_latest_do_not_synchronize(monkeypatch):
    (gpu, _), (gs, _) = _pair([torch.float32], [1], [1])
    gs[0].fill_(3.0)
    gpu.update()
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a host synchronisation inside snapshot() / latest()")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", boom)
        mp.setattr(torch.cuda.Event, "synchronize", boom)
        mp.setattr(torch.cuda.Stream, "synchronize", boom)
        assert gpu.latest() == {}
        gpu.snapshot()
        first = gpu.latest()  # the copy may or may not have arrived: either answer, no stall
        assert first == {} or first["m0"].count == 1
    torch.cuda.current_stream().synchronize()
    got = gpu.latest()
    assert got["m0"].val == 3.0 and got["m0"].count == 1 and gpu.latest_calls == 1


def test_two_snapshots_in_flight_keep_the_older_one():
    (gpu, _), (gs, _) = _pair([torch.float32], [1], [1])
    gs[0].fill_(1.0)
    gpu.update()
    gpu.snapshot()  # A
    gpu.update()
    gpu.snapshot()  # B, enqueued behind A into the OTHER pinned buffer
    torch.cuda.current_stream().synchronize()
    a, b = gpu._pinned[1], gpu._pinned[0]
    assert a.data_ptr() != b.data_ptr() and a.is_pinned() and b.is_pinned()
    assert int(a[-1]) == 1 and int(b[-1]) == 2  # B's copy did not land on A

    class InFlight:  # B's event as it looks while its copy has not completed
        def query(self):
            return False

        def synchronize(self):
            raise AssertionError("latest() waited")

    real, gpu._events[0] = gpu._events[0], InFlight()
    got = gpu.latest()
    assert gpu.latest_calls == 1 and got["m0"].count == 1  # the older snapshot is what is readable
    gpu._events[0] = real
    got = gpu.latest()
    assert gpu.latest_calls == 2 and got["m0"].count == 2
