"""The learning-rate schedule inside the fused update on the GPU: FusedAdamW.attach_schedule(scheduler) uploads the schedule, and
every update call (mtlora_adamw_sched_update_dev) takes each group's lr from it at a count of update calls the kernels keep
themselves; GraphedTrainStep(lr_scheduler=) captures that, so a replay needs nothing from the host.

What the device is held to:
* the lr of update call n is the host scheduler's ``_get_lr(max(n - 1, 0))`` (the reference steps its scheduler after the optimizer):
  bit for bit where the value is formed with + - * / alone (warm-up, the whole linear kind, the lr_min plateau), within a relative
  2^-40 where the device's cos / pow come in -- a condition, not a measurement: it keeps the fp32 value the step kernel consumes
  within one fp32 ulp (2^-23) of the host's;
* everything else bit for bit against the EXISTING kernels: a second, schedule-free FusedAdamW(capturable=True) that is fed the
  doubles read back from ``lr_used()`` as ``param_groups["lr"]``, on the same gradients.

Shapes: three tensors of 1, 4097 and 10000 elements in two groups (they straddle one MTLORA_ADAMW_CHUNK), seeded fp32 gradients,
16 update calls.  Schedule settings as tests/test_cpu_lr_scheduler.py.  The largest relative lr difference seen per kind is printed
and appended to the file named by MTLORA_OPTIM_FIGURES when that is set.
"""
import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.05
BASE = [5e-4, 5e-5]
WARMUP_T, WARMUP_LR_INIT, T_INITIAL, LR_MIN, LR_MIN_RATE = 3, 1e-7, 12, 1e-6, 0.01
DECAY_T, DECAY_RATE, MILESTONES, GAMMA = 4, 0.5, [5, 9], 0.1
KINDS = ["cosine", "cosine_prefix", "step", "linear", "multistep"]
# (test ids: "lin", not "linear" -- conftest runs every GPU test whose NAME holds "linear" once per MTLoRALinear kernel family)
KIND_IDS = ["cosine", "cosine_prefix", "step", "lin", "multistep"]
NUMELS = [1, 4097, 10000]
CALLS = 16
INIT_SCALE = 2.0 ** 10
RTOL = 2.0 ** -40

_FIGURES = []


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("MTLORA_OPTIM_FIGURES")
    if path and _FIGURES:
        with open(path, "a") as f:
            f.write("\n".join(_FIGURES) + "\n")


def dev():
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def scheduler_for(kind, opt):
    from mtlora_amd import lr_scheduler as S
    common = dict(warmup_t=WARMUP_T, warmup_lr_init=WARMUP_LR_INIT, t_in_epochs=False)
    if kind in ("cosine", "cosine_prefix"):
        return S.CosineLRScheduler(opt, t_initial=T_INITIAL, lr_min=LR_MIN, warmup_prefix=(kind == "cosine_prefix"), **common)
    if kind == "step":
        return S.StepLRScheduler(opt, decay_t=DECAY_T, decay_rate=DECAY_RATE, **common)
    if kind == "linear":
        return S.LinearLRScheduler(opt, t_initial=T_INITIAL, lr_min_rate=LR_MIN_RATE, **common)
    return S.MultiStepLRScheduler(opt, milestones=list(MILESTONES), gamma=GAMMA, **common)


def make(kind=None, with_scaler=False, values=None, attach=True):
    """parameters (seeded, or copies of ``values``), a capturable FusedAdamW over two groups, and -- with ``kind`` -- its scheduler,
    attached unless ``attach`` is False"""
    from mtlora_amd.optim import FusedAdamW, LossScaler
    g = torch.Generator().manual_seed(7)
    init = [torch.randn(n, generator=g) for n in NUMELS] if values is None else values
    ps = [torch.nn.Parameter(t.detach().clone().to(dev())) for t in init]
    groups = [{"params": [ps[0], ps[2]]}, {"params": [ps[1]], "lr": BASE[1], "weight_decay": 0.0}]
    opt = FusedAdamW(groups, lr=BASE[0], betas=BETAS, eps=EPS, weight_decay=WD, capturable=True)
    sched = scheduler_for(kind, opt) if kind else None
    if sched is not None and attach:
        opt.attach_schedule(sched)
    return ps, opt, sched, (LossScaler(init_scale=INIT_SCALE) if with_scaler else None)


def grads_of(j, scaled=False, inf=False):
    g = torch.Generator().manual_seed(100 + j)
    out = [torch.randn(n, generator=g) * (0.05 * (INIT_SCALE if scaled else 1.0)) for n in NUMELS]
    if inf:
        out[1][NUMELS[1] - 1] = float("inf")  # the one-element tail chunk of the 4097-element tensor
    return [t.to(dev()) for t in out]


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g


def set_lr(opt, lrs):
    for g, lr in zip(opt.param_groups, lrs):
        g["lr"] = lr


def snapshot(ps, opt):
    torch.cuda.synchronize()
    return {"params": [p.detach().clone() for p in ps], "m": opt._exp_avg.clone(), "v": opt._exp_avg_sq.clone(),
            "ctrl": opt._ctrl.clone()}


def assert_same(got, want, what):
    """parameters, exp_avg, exp_avg_sq and ctrl[0..4] (norm, found_inf, clip coefficient, its unscaled form, Adam's t)"""
    for i, (a, b) in enumerate(zip(got["params"], want["params"])):
        assert same(a, b), f"{what}: parameter {i}"
    assert same(got["m"], want["m"]) and same(got["v"], want["v"]), f"{what}: state"
    assert same(got["ctrl"][:5], want["ctrl"][:5]), f"{what}: ctrl {got['ctrl'][:5].tolist()} vs {want['ctrl'][:5].tolist()}"


def check_lr(kind, sched, n, used):
    """``used`` (Python floats read back after update call n) against the host scheduler; returns the largest relative difference"""
    t = max(n - 1, 0)
    want = sched._get_lr(t)
    worst = 0.0
    for g, (a, b) in enumerate(zip(used, want)):
        if t < WARMUP_T or kind == "linear" or b == LR_MIN:
            assert a == b, f"{kind}: update {n} group {g}: {a!r} != {b!r} (exact segment)"
        else:
            rel = abs(a - b) / abs(b)
            assert rel <= RTOL, f"{kind}: update {n} group {g}: {a!r} vs {b!r}, relative {rel:.3e} > 2^-40"
            worst = max(worst, rel)
    return worst


@functools.lru_cache(maxsize=None)
def trajectory(kind):
    """16 update calls with the schedule attached, and next to them the schedule-free optimizer fed lr_used(): computed once per
    kind, left unchanged"""
    ps, opt, sched, _ = make(kind)
    twin_ps, twin, _, _ = make()
    assert opt.num_updates().item() == 0 and opt.lr_used().tolist() == [0.0, 0.0]
    out = []
    for n in range(CALLS):
        set_grads(ps, grads_of(n))
        norm = opt.clip_and_step(5.0)
        used = opt.lr_used().tolist()  # (synchronises)
        set_lr(twin, used)
        set_grads(twin_ps, grads_of(n))
        twin_norm = twin.clip_and_step(5.0)
        out.append(dict(used=used, u=opt.num_updates().item(), snap=snapshot(ps, opt), twin=snapshot(twin_ps, twin),
                        norm=norm.clone(), twin_norm=twin_norm.clone()))
    return sched, out


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lr_sequence(kind):
    """1. lr_used() after update n is _get_lr(max(n - 1, 0)): exact on the warm-up, the linear kind and the lr_min plateau, within
    2^-40 relative elsewhere; the counter reads n + 1"""
    sched, out = trajectory(kind)
    worst = 0.0
    for n, o in enumerate(out):
        assert o["u"] == n + 1
        worst = max(worst, check_lr(kind, sched, n, o["used"]))
    _FIGURES.append(f"lr schedule {kind}: largest relative difference device vs host over {CALLS} updates {worst:.3e} (bound 2^-40 = {RTOL:.3e})")
    print(_FIGURES[-1])
    if kind == "cosine":  # the plateau is reached inside the 16 calls: t = 12 .. 14
        assert out[13]["used"] == [LR_MIN, LR_MIN] and out[15]["used"] == [LR_MIN, LR_MIN]
    assert out[0]["used"] == out[1]["used"] == [WARMUP_LR_INIT] * 2  # update 0 at the constructor's value, update 1 at _get_lr(0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_update_bits(kind):
    """2. after every call parameters, exp_avg, exp_avg_sq and ctrl[0..4] are bit-identical to the schedule-free optimizer given the
    doubles of lr_used() -- the schedule path is the existing kernels"""
    _, out = trajectory(kind)
    for n, o in enumerate(out):
        assert_same(o["snap"], o["twin"], f"{kind}: update {n}")
        assert same(o["norm"], o["twin_norm"])
    # Adam's t counts the calls whose lr is usable: the linear kind runs below zero behind t_initial (here from t = 13 on, updates 14
    # and 15), and a negative lr skips the step on the device as it is refused on the by-value path -- on both optimizers alike
    sched = trajectory(kind)[0]
    steps = sum(1 for n in range(CALLS) if min(sched._get_lr(max(n - 1, 0))) >= 0.0)
    assert steps == (14 if kind == "linear" else CALLS)
    assert out[-1]["snap"]["ctrl"][4].item() == steps and not same(out[-1]["snap"]["params"][2], out[0]["snap"]["params"][2])


def test_accumulation():
    """3. k = 3, 12 calls: the counter reads 0, 0, 1, 1, 1, 2, ...; lr_used moves on calls 3, 6, 9, 12 only; on the others the
    counter, lr_used, parameters and state are bitwise unchanged; the result is the schedule-free optimizer's on the torch-formed
    sums ((g0 + g1) + g2) at the lr read back"""
    k = 3
    ps, opt, sched, _ = make("linear")
    twin_ps, twin, _, _ = make()
    buf = opt._sched_dev
    for call in range(1, 13):
        before, before_buf = snapshot(ps, opt), buf.clone()
        set_grads(ps, grads_of(call - 1))
        opt.clip_and_step(5.0, None, accumulation_steps=k)
        opt.zero_grad(set_to_none=True)
        after = snapshot(ps, opt)
        assert opt.num_updates().item() == call // k, call
        if call % k:
            assert torch.equal(buf, before_buf), f"call {call}: the schedule buffer moved"
            assert_same(after, before, f"call {call}")
            continue
        n = call // k - 1
        used = opt.lr_used().tolist()
        check_lr("linear", sched, n, used)
        assert not torch.equal(buf, before_buf)
        js = list(range(call - k, call))
        tot = grads_of(js[0])
        for j in js[1:]:
            tot = [a + b for a, b in zip(tot, grads_of(j))]
        set_lr(twin, used)
        set_grads(twin_ps, tot)
        twin.clip_and_step(5.0)
        assert_same(after, snapshot(twin_ps, twin), f"update {n}")
    assert opt._ctrl[4].item() == 4.0 and opt.lr_used().tolist() == sched._get_lr(2)


def test_skipped_step():
    """4. one call with an inf gradient, under a LossScaler: the counter of update CALLS advances, Adam's step counter and the
    parameters do not, the scale backs off, and the next call's lr is the schedule's next value"""
    ps, opt, sched, scaler = make("linear", with_scaler=True)
    for n in range(2):
        set_grads(ps, grads_of(n, scaled=True))
        opt.clip_and_step(5.0, scaler)
    before = snapshot(ps, opt)
    scale = scaler._scale.item()
    assert before["ctrl"][4].item() == 2.0 and opt.num_updates().item() == 2 and scale == INIT_SCALE
    set_grads(ps, grads_of(2, scaled=True, inf=True))
    norm = opt.clip_and_step(5.0, scaler)
    after = snapshot(ps, opt)
    assert not math.isfinite(norm.item()) and after["ctrl"][1].item() == 1.0
    assert opt.num_updates().item() == 3 and after["ctrl"][4].item() == 2.0
    for a, b in zip(after["params"], before["params"]):
        assert same(a, b)
    assert same(after["m"], before["m"]) and same(after["v"], before["v"])
    assert scaler._scale.item() == 0.5 * scale and scaler._growth_tracker.item() == 0
    assert opt.lr_used().tolist() == sched._get_lr(1)  # the skipped call had its lr all the same
    set_grads(ps, grads_of(3, scaled=True))
    norm = opt.clip_and_step(5.0, scaler)
    assert math.isfinite(norm.item()) and opt.lr_used().tolist() == sched._get_lr(2) and opt.num_updates().item() == 4
    assert opt._ctrl[4].item() == 3.0 and not same(ps[2], before["params"][2])


def test_bad_record_skips_the_step():
    """5. a nan lr_min written into the device record behind the host check's back: the kernel's own validation raises found_inf
    -- the step is skipped, the norm is nan, the parameters stay; with the value put back the next call steps again"""
    from mtlora_amd import _lib
    ps, opt, sched, _ = make("cosine")
    for n in range(2):
        set_grads(ps, grads_of(n))
        opt.clip_and_step(5.0)
    before = snapshot(ps, opt)
    word = opt._sched_dev.view(torch.float64)[_lib.LrSchedule.lr_min.offset // 8:_lib.LrSchedule.lr_min.offset // 8 + 1]
    assert word.item() == LR_MIN
    word.fill_(float("nan"))
    set_grads(ps, grads_of(2))
    norm = opt.clip_and_step(5.0)
    after = snapshot(ps, opt)
    assert math.isnan(norm.item()) and after["ctrl"][1].item() == 1.0 and after["ctrl"][4].item() == before["ctrl"][4].item() == 2.0
    for a, b in zip(after["params"], before["params"]):
        assert same(a, b)
    assert same(after["m"], before["m"]) and same(after["v"], before["v"])
    assert all(math.isnan(x) for x in opt.lr_used().tolist()) and opt.num_updates().item() == 3
    word.fill_(LR_MIN)
    set_grads(ps, grads_of(3))
    norm = opt.clip_and_step(5.0)
    assert math.isfinite(norm.item()) and opt._ctrl[4].item() == 3.0 and opt.lr_used().tolist() == sched._get_lr(2)
    assert not same(ps[2], before["params"][2])


def test_resume():
    """6. 7 calls, state_dict(), then a fresh optimizer + scheduler + load_state_dict + attach_schedule for 9 more calls: bit-identical
    to 16 uninterrupted calls (the count of update calls travels under "lr_schedule_updates"; a state without the key loads as
    before and the schedule starts from the scheduler's own count)"""
    _, whole = trajectory("linear")
    ps, opt, sched, _ = make("linear")
    for n in range(7):
        set_grads(ps, grads_of(n))
        opt.clip_and_step(5.0)
    sd = opt.state_dict()
    assert sd["lr_schedule_updates"] == 7 and set(sd) == {"state", "param_groups", "lr_schedule_updates"}
    ps2, opt2, sched2, _ = make("linear", values=[p.detach().cpu() for p in ps], attach=False)
    opt2.load_state_dict(sd)
    opt2.attach_schedule(sched2)
    assert opt2.num_updates().item() == 7 and opt2._ctrl[4].item() == 7.0
    for n in range(7, CALLS):
        set_grads(ps2, grads_of(n))
        opt2.clip_and_step(5.0)
        assert_same(snapshot(ps2, opt2), whole[n]["snap"], f"resumed update {n}")
        assert opt2.lr_used().tolist() == whole[n]["used"] and opt2.num_updates().item() == whole[n]["u"]
    # without the key: as a checkpoint of the parent commit loads; the count then comes from the scheduler (a fresh one: 0)
    del sd["lr_schedule_updates"]
    ps3, opt3, sched3, _ = make("linear", values=[p.detach().cpu() for p in ps], attach=False)
    opt3.load_state_dict(sd)
    opt3.attach_schedule(sched3)
    assert opt3.num_updates().item() == 0 and opt3._ctrl[4].item() == 7.0
    sched3.step_update(6)  # what the reference's loop had called last after 7 updates
    opt3.attach_schedule(sched3)
    assert opt3.num_updates().item() == 7
    opt3.attach_schedule(sched3, num_updates=11)
    assert opt3.num_updates().item() == 11


def test_detach():
    """8. after detach_schedule() the next call uses param_groups["lr"] and matches the schedule-free optimizer bit for bit"""
    ps, opt, sched, _ = make("step")
    twin_ps, twin, _, _ = make()
    for n in range(3):
        set_grads(ps, grads_of(n))
        opt.clip_and_step(5.0)
        set_lr(twin, opt.lr_used().tolist())
        set_grads(twin_ps, grads_of(n))
        twin.clip_and_step(5.0)
    opt.detach_schedule()
    with pytest.raises(RuntimeError, match="no schedule"):
        opt.lr_used()
    buf = opt._sched_dev.clone()
    for n, lrs in ((3, [1.23e-4, 0.5e-4]), (4, [1.23e-4, 0.5e-4]), (5, [2e-4, 1e-4])):
        for o, q in ((opt, ps), (twin, twin_ps)):
            set_lr(o, lrs)
            set_grads(q, grads_of(n))
            o.clip_and_step(5.0)
        assert_same(snapshot(ps, opt), snapshot(twin_ps, twin), f"detached call {n}")
    assert torch.equal(opt._sched_dev, buf)  # the schedule buffer is no longer touched
    assert "lr_schedule_updates" not in opt.state_dict()


# ---- 7. in the graph -----------------------------------------------------------------------------------------------------------
TASKS = ["semseg", "normals", "sal", "human_parts"]
MODEL_KW = dict(img_size=224, tasks=TASKS, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4)  # test_gpu_optim_capturable's
REPLAYS = 8


def graphed_run(kind, k, on_device):
    """one GraphedTrainStep (the fp16 step with a LossScaler of test_gpu_optim_capturable) from a fixed seed, replayed REPLAYS
    times; ``on_device``: the schedule is inside the graph, else the host scheduler's step_update runs in front of every replay.
    Returns per replay the loss, the trainable parameters, lr_used (device leg) and whether push_hyperparameters() uploaded."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW, LossScaler
    torch.manual_seed(9)
    Fn._seed_counter = 0
    img, tg = H.synthetic_batch(2, 224, TASKS, seed=17, device=dev())
    model = H.build_model(**MODEL_KW).to(dev()).train()
    crit, opt = H.MultiTaskLoss(TASKS), H.build_optimizer(model, lr=BASE[0], impl="hip", capturable=True)
    assert isinstance(opt, FusedAdamW)
    base = [g["lr"] for g in opt.param_groups]
    sched = scheduler_for(kind, opt)
    assert sched.base_values == base
    scaler = LossScaler(init_scale=INIT_SCALE)
    try:
        gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16, loss_scaler=scaler,
                                accumulation_steps=k, lr_scheduler=sched if on_device else None)
        assert gs.graphed is True and gs.why == "", gs.why
        assert opt._ctrl[4].item() == 2.0  # two warm-up steps, both update calls: at _get_lr(0), the constructor's value
        if on_device:
            assert opt.num_updates().item() == 2
        trainable = [p for p in model.parameters() if p.requires_grad]
        rows = []
        for c in range(REPLAYS):
            n = 2 + c // k  # the index of the update call this replay belongs to
            sched.step_update(n - 1)  # device leg: harmless, moves param_groups["lr"] for logging only
            pushed = opt.push_hyperparameters()
            loss = gs()
            torch.cuda.synchronize()
            rows.append(dict(loss=loss.clone(), params=[p.detach().clone() for p in trainable], pushed=pushed, n=n,
                             updated=gs.updated, used=opt.lr_used().tolist() if on_device else None,
                             u=opt.num_updates().item() if on_device else None))
        return sched, rows
    finally:
        Fn.set_seed_offset(None)


@pytest.mark.parametrize("k", [1, 2], ids=["k1", "k2"])
def test_graphed_step_with_the_schedule_inside(k):
    """GraphedTrainStep(lr_scheduler=linear) against a second GraphedTrainStep from the same seed whose host scheduler calls
    step_update between replays: loss and every trainable parameter bit-identical after each of 8 replays (the linear kind is
    exact), with no push_hyperparameters() upload on the device leg after the first replay -- while the host leg uploads"""
    sched, got = graphed_run("linear", k, on_device=True)
    _, want = graphed_run("linear", k, on_device=False)
    assert not any(r["pushed"] for r in got[1:]), [r["pushed"] for r in got]
    assert any(r["pushed"] for r in want)
    for c, (a, b) in enumerate(zip(got, want)):
        assert a["updated"] == b["updated"] == ((c + 1) % k == 0)
        assert torch.equal(a["loss"], b["loss"]) and torch.isfinite(a["loss"]).all(), f"replay {c}: loss {a['loss'].item()} vs {b['loss'].item()}"
        for i, (p, q) in enumerate(zip(a["params"], b["params"])):
            assert same(p, q), f"replay {c}: trainable parameter {i}"
        if a["updated"]:
            assert a["u"] == a["n"] + 1
            check_lr("linear", sched, a["n"], a["used"])
    assert not same(got[-1]["params"][0], got[0]["params"][0]) or not same(got[-1]["params"][-1], got[0]["params"][-1])


def test_graphed_step_cosine_lr_sequence():
    """the cosine kind inside the graph: only the lr_used sequence is compared (cos is the device library's), as in check 1"""
    sched, got = graphed_run("cosine", 1, on_device=True)
    assert not any(r["pushed"] for r in got[1:])
    worst = 0.0
    for r in got:
        assert r["u"] == r["n"] + 1
        worst = max(worst, check_lr("cosine", sched, r["n"], r["used"]))
    _FIGURES.append(f"lr schedule cosine, replayed: largest relative difference device vs host {worst:.3e} (bound 2^-40 = {RTOL:.3e})")
    print(_FIGURES[-1])
