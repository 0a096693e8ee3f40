"""Gradient accumulation inside the fused update on the GPU: FusedAdamW.clip_and_step(accumulation_steps=k) is one micro-step
(mtlora_adamw_accum_update_dev) -- the gradients are summed into a persistent fp32 accumulator and a device counter lets only every
k-th call clip, step and update the scaler -- and GraphedTrainStep(accumulation_steps=k) replays that as ONE graph.

The definition the kernel level is held to: k calls with g_0 .. g_(k-1) give, bit for bit, what ONE step of the existing path
(mtlora_adamw_update_dev) gives on ((g_0 + g_1) + g_2) formed by torch in fp32.  Those references are computed once per (k, scaler)
and left unchanged; every comparison is on the bit patterns.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.05
INIT_SCALE = 2.0 ** 10
LR = 1e-3
# chunk boundary (4096) and tails shorter than a 16-byte access; index 6: parameter AND gradient at a 4-byte, not 16-byte, aligned
# address, two chunks long (the scalar paths of both kernels); index 7: never has a gradient
NUMELS = [1, 3, 4095, 4096, 4097, 10000, 4101, 7]
MISALIGNED, NO_GRAD = 6, 7


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def off_by_one(t):
    """a copy of ``t`` whose first element sits 4 bytes behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    out = buf[1:]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def make(with_scaler, capturable=True, init_scale=INIT_SCALE):
    from mtlora_amd.optim import FusedAdamW, LossScaler
    g = torch.Generator().manual_seed(7)
    ps = []
    for i, n in enumerate(NUMELS):
        t = torch.randn(n, generator=g).to(dev())
        ps.append(torch.nn.Parameter(off_by_one(t) if i == MISALIGNED else t))
    assert ps[MISALIGNED].data_ptr() % 16 == 4
    groups = [{"params": ps[0::2]}, {"params": ps[1::2], "weight_decay": 0.0, "lr": 0.3 * LR}]
    opt = FusedAdamW(groups, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, capturable=capturable)
    return ps, opt, (LossScaler(init_scale=init_scale) if with_scaler else None)


def grads_of(j, with_scaler, inf=False):
    """the (loss-scaled) gradients of micro-step j, seeded; None for the tensor that never has one; ``inf``: one inf, in the
    last element of the 4097-element tensor (the one-element tail chunk)"""
    g = torch.Generator().manual_seed(100 + j)
    mul = 0.05 * (INIT_SCALE if with_scaler else 1.0)
    out = [torch.randn(n, generator=g) * mul for n in NUMELS]
    if inf:
        out[4][NUMELS[4] - 1] = float("inf")
    out = [t.to(dev()) for t in out]
    out[MISALIGNED] = off_by_one(out[MISALIGNED])
    out[NO_GRAD] = None
    return out


def summed(js, with_scaler):
    """((g_0 + g_1) + g_2): one fp32 add per element, in micro-step order, by torch"""
    tot = grads_of(js[0], with_scaler)
    for j in js[1:]:
        tot = [None if a is None else a + b for a, b in zip(tot, grads_of(j, with_scaler))]
    return tot


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g


def snapshot(ps, opt, scaler, norm=None):
    torch.cuda.synchronize()
    s = {"params": [p.detach().clone() for p in ps], "m": opt._exp_avg.clone(), "v": opt._exp_avg_sq.clone(),
         "ctrl": opt._ctrl.clone()}
    if norm is not None:
        s["norm"] = norm.clone()
    if scaler is not None:
        s["scale"], s["tracker"] = scaler._scale.clone(), scaler._growth_tracker.clone()
    return s


def assert_same(got, want, what, ctrl=slice(0, 5)):
    """parameters, both state buffers, ctrl[0..4] (norm, found_inf, clip coefficient, its unscaled form, t), the bias corrections
    behind them, the norm word and the scaler's two words"""
    for i, (a, b) in enumerate(zip(got["params"], want["params"])):
        assert same(a, b), f"{what}: parameter {i}"
    assert same(got["ctrl"][ctrl], want["ctrl"][ctrl]), f"{what}: ctrl {got['ctrl'][:8].tolist()} vs {want['ctrl'][:8].tolist()}"
    assert same(got["ctrl"][8:], want["ctrl"][8:]), f"{what}: bias corrections"
    for k in ("m", "v", "norm", "scale", "tracker"):
        if k in want and k in got:
            assert same(got[k], want[k]), f"{what}: {k} {got[k].flatten()[:8].tolist()} vs {want[k].flatten()[:8].tolist()}"


def micro(opt):
    from mtlora_amd import _lib
    return opt._ctrl[_lib.ADAMW_CTRL_MICRO].item(), opt._ctrl[_lib.ADAMW_CTRL_UPDATED].item()


@functools.lru_cache(maxsize=None)
def definition(k, with_scaler):
    """two steps of the existing path (clip_and_step without accumulation_steps) on the torch-formed sums of two cycles: the
    reference, computed once per (k, scaler)"""
    ps, opt, scaler = make(with_scaler)
    snaps = []
    for cycle in range(2):
        set_grads(ps, summed(list(range(cycle * k, (cycle + 1) * k)), with_scaler))
        snaps.append(snapshot(ps, opt, scaler, opt.clip_and_step(5.0, scaler)))
    assert snaps[1]["ctrl"][4].item() == 2.0 and snaps[1]["ctrl"][1].item() == 0.0 and torch.isfinite(snaps[1]["norm"])
    assert not same(snaps[0]["params"][5], snaps[1]["params"][5]) and ps[NO_GRAD] not in opt.state
    return snaps


@pytest.mark.parametrize("with_scaler", [False, True], ids=["noscaler", "scaler"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_accumulated_cycle_equals_one_step_on_the_sum(k, with_scaler):
    """1. bitwise against the definition, over two full cycles: the second one starts with the first one's sums still in the
    accumulator, so the overwrite at c == 0 is what makes it pass"""
    ps, opt, scaler = make(with_scaler)
    for cycle in range(2):
        for j in range(cycle * k, (cycle + 1) * k):
            set_grads(ps, grads_of(j, with_scaler))
            norm = opt.clip_and_step(5.0, scaler, accumulation_steps=k)
            opt.zero_grad(set_to_none=True)
        assert_same(snapshot(ps, opt, scaler, norm), definition(k, with_scaler)[cycle], f"k={k} cycle {cycle + 1}")
        if k > 1:
            assert micro(opt) == (0.0, 1.0)
    if k > 1:
        assert opt._acc.dtype == torch.float32 and opt._acc.numel() == sum(-(-n // 4) * 4 for n in NUMELS)
        sd = opt.state_dict()  # torch AdamW's keys; neither the accumulator nor the counter travels
        assert set(sd) == {"state", "param_groups"}
        assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    assert ps[NO_GRAD] not in opt.state and same(ps[NO_GRAD], make(with_scaler)[0][NO_GRAD])


@pytest.mark.parametrize("with_scaler", [False, True], ids=["noscaler", "scaler"])
@pytest.mark.parametrize("k", [2, 3])
def test_accumulating_micro_steps_write_nothing(k, with_scaler):
    """2. after each of the first k - 1 calls of a cycle (the second cycle: state, norm and counter are no longer zero), the
    parameters, exp_avg, exp_avg_sq, the whole control block up to the counter, the scaler's words and the norm word are bitwise
    what they were, and the counter reads 1, 2, ..."""
    ps, opt, scaler = make(with_scaler)
    for j in range(k):
        set_grads(ps, grads_of(j, with_scaler))
        norm = opt.clip_and_step(5.0, scaler, accumulation_steps=k)
    before = snapshot(ps, opt, scaler, norm)
    assert before["ctrl"][4].item() == 1.0 and before["norm"].item() > 0.0
    for j in range(k, 2 * k - 1):
        set_grads(ps, grads_of(j, with_scaler))
        assert opt.clip_and_step(5.0, scaler, accumulation_steps=k) is norm  # the persistent word of the last update
        assert_same(snapshot(ps, opt, scaler, norm), before, f"k={k} micro-step {j - k + 1}")
        assert micro(opt) == (float(j - k + 1), 0.0)
    set_grads(ps, grads_of(2 * k - 1, with_scaler))
    opt.clip_and_step(5.0, scaler, accumulation_steps=k)
    assert_same(snapshot(ps, opt, scaler, norm), definition(k, with_scaler)[1], f"k={k} update")
    assert micro(opt) == (0.0, 1.0)


def test_one_step_cycle_equals_the_parent_path():
    """3. accum_steps == 1 through the library entry itself (FusedAdamW takes the existing call for k = 1) against the by-value
    path, the parent's clip_and_step: p, m, v, ctrl[0..4], norm, scale and tracker bitwise, over two steps; the accumulator is
    not written"""
    from mtlora_amd import _lib
    ref_ps, ref_opt, ref_scaler = make(True, capturable=False)
    ps, opt, scaler = make(True)
    opt.prepare_accumulation()
    opt._acc.fill_(-3.0)
    scaler._lazy_init(dev())
    norm = torch.zeros((), device=dev())
    for j in range(2):
        set_grads(ref_ps, grads_of(j, True))
        want = snapshot(ref_ps, ref_opt, ref_scaler, ref_opt.clip_and_step(5.0, ref_scaler))
        set_grads(ps, grads_of(j, True))
        # the table is in the optimizer's order (group by group), and so is the pointer array
        ptrs = torch.tensor([0 if p.grad is None else p.grad.data_ptr() for p in opt._params], dtype=torch.int64).to(dev())
        opt.push_hyperparameters()
        rc = _lib.lib().mtlora_adamw_accum_update_dev(
            opt._table.data_ptr(), ptrs.data_ptr(), len(ps), opt._n_chunks, opt._hyper_dev.data_ptr(), len(opt.param_groups), 5.0,
            opt._ctrl.data_ptr(), norm.data_ptr(), scaler._scale.data_ptr(), scaler._growth_tracker.data_ptr(), scaler._growth_factor,
            scaler._backoff_factor, scaler._growth_interval, opt._scratch.data_ptr(), opt._scratch_bytes, opt._acc.data_ptr(),
            opt._acc_offsets.data_ptr(), 1, _lib.stream_ptr())
        assert rc == 0
        assert_same(snapshot(ps, opt, scaler, norm), want, f"step {j + 1}")
        assert micro(opt) == (0.0, 1.0)
    assert bool((opt._acc == -3.0).all())


def test_inf_skips_the_cycle_and_leaves_no_trace():
    """4. k = 3 with a scaler, one inf in g_1 of the second cycle: at the third call the step is skipped (p, m, v, t bitwise
    unchanged, the scale backed off once, tracker 0, counter 0); the next clean cycle is bitwise the same cycle run by a second
    optimizer that never saw the inf and holds the same p / m / v / t and the backed-off scale"""
    k = 3
    ps, opt, scaler = make(True)
    twin_ps, twin_opt, twin_scaler = make(True)
    for j in range(k):  # one good cycle on both: non-trivial state
        for q, o, s in ((ps, opt, scaler), (twin_ps, twin_opt, twin_scaler)):
            set_grads(q, grads_of(j, True))
            o.clip_and_step(5.0, s, accumulation_steps=k)
    norm = opt._accum_norm
    before = snapshot(ps, opt, scaler, norm)
    assert_same(before, definition(k, True)[0], "good cycle")
    for j in range(k):
        set_grads(ps, grads_of(10 + j, True, inf=(j == 1)))
        opt.clip_and_step(5.0, scaler, accumulation_steps=k)
    after = snapshot(ps, opt, scaler, norm)
    for a, b in zip(after["params"], before["params"]):
        assert same(a, b)
    assert same(after["m"], before["m"]) and same(after["v"], before["v"])
    assert after["ctrl"][4].item() == before["ctrl"][4].item() == 1.0 and after["ctrl"][1].item() == 1.0
    assert same(after["ctrl"][8:], before["ctrl"][8:])
    assert after["scale"].item() == 0.5 * before["scale"].item() and after["tracker"].item() == 0
    assert not math.isfinite(after["norm"].item()) and micro(opt) == (0.0, 1.0)
    at = opt._acc_offsets[[id(p) for p in opt._params].index(id(ps[4]))].item()  # (slices are in the optimizer's order)
    assert not bool(torch.isfinite(opt._acc[at:at + NUMELS[4]]).all())  # the poison is in acc
    twin_scaler._scale.fill_(0.5 * before["scale"].item())
    twin_scaler._growth_tracker.fill_(0)
    for j in range(k):
        for q, o, s in ((ps, opt, scaler), (twin_ps, twin_opt, twin_scaler)):
            set_grads(q, grads_of(20 + j, True))
            o.clip_and_step(5.0, s, accumulation_steps=k)
    got, want = snapshot(ps, opt, scaler, norm), snapshot(twin_ps, twin_opt, twin_scaler, twin_opt._accum_norm)
    assert_same(got, want, "clean cycle after the skipped one")
    assert got["ctrl"][4].item() == 2.0 and got["ctrl"][1].item() == 0.0 and math.isfinite(got["norm"].item())
    assert all(bool(torch.isfinite(p).all()) for p in got["params"]) and bool(torch.isfinite(got["m"]).all())


def test_replayed_cycles_follow_the_learning_rate():
    """5. ONE captured clip_and_step(5.0, scaler, accumulation_steps=2), gradients in static buffers, replayed for two cycles with
    param_groups' lr changed in between (push_hyperparameters() before each replay): bitwise the definition -- one step per cycle
    on the torch-formed sum -- run with the same two learning rates"""
    k, new_lr = 2, (0.37e-3, 0.11e-3)
    ref_ps, ref_opt, ref_scaler = make(True)
    want = []
    for cycle in range(2):
        if cycle == 1:
            ref_opt.param_groups[0]["lr"], ref_opt.param_groups[1]["lr"] = new_lr
        set_grads(ref_ps, summed([2 * cycle, 2 * cycle + 1], True))
        want.append(snapshot(ref_ps, ref_opt, ref_scaler, ref_opt.clip_and_step(5.0, ref_scaler)))
    assert not same(want[1]["params"][5], definition(k, True)[1]["params"][5])  # the new lr shows in the second step

    ps, opt, scaler = make(True)
    init = [p.detach().clone() for p in ps]
    set_grads(ps, [None if g is None else torch.zeros_like(g) for g in grads_of(0, True)])
    ps[MISALIGNED].grad = off_by_one(torch.zeros(NUMELS[MISALIGNED], device=dev()))

    def fill(j):
        for p, g in zip(ps, grads_of(j, True)):
            if g is not None:
                p.grad.copy_(g)

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture stream: allocates the accumulator, pushes the hyper-parameters
        opt.clip_and_step(5.0, scaler, accumulation_steps=k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():  # back to the initial state, in the same buffers (the accumulator keeps the warm-up's values)
        for p, q in zip(ps, init):
            p.copy_(q)
        opt._exp_avg.zero_()
        opt._exp_avg_sq.zero_()
        opt._ctrl.zero_()
        scaler._scale.fill_(INIT_SCALE)
        scaler._growth_tracker.fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = opt.clip_and_step(5.0, scaler, accumulation_steps=k)
    versions = [p._version for p in ps]
    for cycle in range(2):
        if cycle == 1:
            opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = new_lr
        for j in (2 * cycle, 2 * cycle + 1):
            fill(j)
            assert opt.push_hyperparameters() is (cycle == 1 and j == 2)  # uploads only on change
            graph.replay()
            opt.bump_versions(updated=(j % 2 == 1))
        assert_same(snapshot(ps, opt, scaler, norm), want[cycle], f"replayed cycle {cycle + 1}")
        assert micro(opt) == (0.0, 1.0)
    # two updates, two version bumps: the accumulating replays invalidated nothing
    assert [p._version for p in ps[:NO_GRAD]] == [v + 2 for v in versions[:NO_GRAD]] and ps[NO_GRAD]._version == versions[NO_GRAD]
    opt.reset_capture()
    assert micro(opt) == (0.0, 0.0)


def test_counter_returns_to_zero_on_load_and_reset():
    """load_state_dict() and reset_capture() abandon a half-made cycle: the next call overwrites the accumulator"""
    ps, opt, scaler = make(False)
    set_grads(ps, grads_of(0, False))
    opt.clip_and_step(5.0, None, accumulation_steps=3)
    assert micro(opt) == (1.0, 0.0)
    opt.reset_capture()
    assert micro(opt) == (0.0, 0.0)
    opt.clip_and_step(5.0, None, accumulation_steps=3)
    opt.clip_and_step(5.0, None, accumulation_steps=3)
    assert micro(opt) == (2.0, 0.0)
    opt.load_state_dict(opt.state_dict())
    assert micro(opt) == (0.0, 0.0)
    for j in range(2):  # a k = 2 cycle from here is the definition's first step
        set_grads(ps, grads_of(j, False))
        norm = opt.clip_and_step(5.0, None, accumulation_steps=2)
    assert_same(snapshot(ps, opt, None, norm), definition(2, False)[0], "cycle after load_state_dict")


def test_whole_step_graphed_with_accumulation():
    """the whole fp16 train step of test_gpu_optim_capturable.test_whole_step_graphed_with_scaler captured with
    accumulation_steps=2: four micro-steps on two alternating batches copied into the static buffers, lr changed after the first
    update, against the eager train_step(..., loss_scaler=, update_grad=(i + 1) % 2 == 0) from the same state with the same
    dropout seeds and offsets.  Criterion, that test's own and for its reason (hipBLASLt may pick another algorithm under
    capture, so not bit-equal): the four losses and the two gradient norms within 2e-3 relative, cosine of the accumulated updates
    >= 0.98.  In addition: the step is a graph; ``updated`` reads False, True, False, True; after micro-steps 1 and 3 every
    trainable parameter is bitwise what it was; an eval forward equals that of a fresh model loaded from the state_dict
    (bump_versions reached the weight caches after the updating replays).

    The k = 2 run must also differ from a graphed k = 1 run on the same four batches and learning rates (a guard against a
    silent "step every call"): it takes two optimizer steps where k = 1 takes four, and its updates are further from k = 1's than
    two runs of the SAME computation may be from each other under the criterion above -- cosine 0.98 at equal length is a relative
    distance of sqrt(2 - 2 * 0.98) = 0.2, so the distance asked for is more than 0.2 (two AdamW steps of ~lr per element against
    four: about half of k = 1's length is expected)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW, LossScaler
    tasks = ["semseg", "normals", "sal", "human_parts"]
    batches = [H.synthetic_batch(2, 224, tasks, seed=s, device=dev()) for s in (17, 18)]
    lrs = [1e-3 * f for f in (0.25, 0.25, 1.0, 1.0)]  # the value in force at micro-step i: it changes after the first update
    kw = dict(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4)
    out = {}
    for mode, k in (("graph", 2), ("eager", 2), ("graph1", 1)):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(**kw).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        assert isinstance(opt, FusedAdamW)
        scaler = LossScaler(init_scale=2.0 ** 10)
        img, tg = batches[0][0].clone(), {t: v.clone() for t, v in batches[0][1].items()}
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16, loss_scaler=scaler,
                                    accumulation_steps=k)
            assert gs.graphed is True and gs.why == "", gs.why
            drawn = Fn._seed_counter  # two warm-up steps and the capture drew the layers' dropout seeds: three equal shares
            assert drawn > 0 and drawn % 3 == 0
            assert opt._ctrl[4].item() == 2.0 and opt._ctrl[5].item() == 0.0  # the warm-up: two plain steps, c untouched
            trainable = {n: p for n, p in model.named_parameters() if p.requires_grad}
            start = {n: p.detach().clone() for n, p in trainable.items()}
            losses, norms, updated = [], [], []
            for i, lr in enumerate(lrs):
                for g in opt.param_groups:
                    g["lr"] = lr
                img.copy_(batches[i % 2][0])
                for t in tg:
                    tg[t].copy_(batches[i % 2][1][t])
                prev = {n: p.detach().clone() for n, p in trainable.items()}
                if mode == "eager":  # the eager step, drawing the seeds the capture drew and walking the same device offset
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                    upd = (i + 1) % k == 0
                    loss, norm = H.train_step(model, crit, opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler,
                                              update_grad=upd)
                else:
                    loss, norm, upd = gs(), gs.grad_norm, gs.updated
                torch.cuda.synchronize()
                updated.append(upd)
                losses.append(loss.clone())
                if upd:
                    norms.append(norm.clone())
                else:
                    assert all(same(p, prev[n]) for n, p in trainable.items()), f"{mode}: micro-step {i + 1} wrote a parameter"
            assert updated == ([False, True, False, True] if k == 2 else [True] * 4), (mode, updated)
            assert opt._ctrl[4].item() == 2.0 + 4 // k  # optimizer steps taken
            out[mode] = (losses, {n: (p.detach() - start[n]).double() for n, p in trainable.items()}, norms)
            if mode == "graph":
                assert opt._ctrl[5].item() == 0.0 and opt._ctrl[6].item() == 1.0
                model.eval()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    got = model(img, upsample=False)
                fresh = H.build_model(**kw)
                fresh.load_state_dict(model.state_dict())
                fresh = fresh.to(dev()).eval()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    want = fresh(img, upsample=False)
                for t in tasks:
                    assert torch.equal(got[t], want[t]), t
        finally:
            Fn.set_seed_offset(None)

    def dot(a, b):
        return sum((a[n] * b[n]).sum().item() for n in a)

    g2, e2, g1 = out["graph"], out["eager"], out["graph1"]
    assert len(g2[0]) == len(e2[0]) == 4 and len(g2[2]) == len(e2[2]) == 2
    for a, b in zip(g2[0], e2[0]):
        print("loss", a.item(), b.item())
        assert abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    for a, b in zip(g2[2], e2[2]):
        print("grad norm", a.item(), b.item())
        assert math.isfinite(a.item()) and abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    cosine = dot(g2[1], e2[1]) / (dot(g2[1], g2[1]) * dot(e2[1], e2[1])) ** 0.5
    print("cosine", cosine)
    assert cosine >= 0.98, cosine
    diff = {n: g2[1][n] - g1[1][n] for n in g1[1]}
    distance = (dot(diff, diff) / dot(g1[1], g1[1])) ** 0.5
    print("relative distance of the k = 2 updates from the k = 1 updates", distance)
    assert distance > 0.2, distance
