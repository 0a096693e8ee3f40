"""The capturable fused update on the GPU: FusedAdamW(capturable=True) reads its hyper-parameters from device memory
(mtlora_adamw_update_dev), so a HIP graph that holds ``clip_and_step`` follows ``param_groups`` from replay to replay, with the
LossScaler inside the graph.

The reference of cases 1 and 2 is the by-value path (capturable=False, eager), computed ONCE per module and left unchanged; the
contract is bit identity, so every comparison is on the bit patterns (which also covers the inf / nan norm of a skipped step).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.05
STEPS, EXTRA = 5, 2          # five steps with a moving lr, then two more with param_groups untouched
INF_STEP = 2                 # "step 3": its gradient holds one inf
INIT_SCALE, GROWTH_INTERVAL = 2.0 ** 10, 2   # (interval 2: the schedule below also crosses a scale growth)


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def numels():
    from mtlora_amd import _lib
    c = _lib.ADAMW_CHUNK  # elements per chunk (MTLORA_ADAMW_CHUNK of optim.hip)
    return [1, 3, c - 1, c, c + 1, 3 * c + 5, 7]  # the last one never has a gradient


def lr_at(k):
    """warm-up ramp (two steps), then a cosine segment, as Python floats; from step STEPS on the value stays"""
    k = min(k, STEPS - 1)
    return 1e-3 * (k + 1) / 2 if k < 2 else 1e-3 * 0.5 * (1.0 + math.cos(math.pi * (k - 1) / 6))


def set_lr(opt, k):
    opt.param_groups[0]["lr"] = lr_at(k)
    opt.param_groups[1]["lr"] = 0.3 * lr_at(k)


def make(capturable):
    from mtlora_amd.optim import FusedAdamW, LossScaler
    g = torch.Generator().manual_seed(7)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev())) for n in numels()]
    groups = [{"params": ps[0::2]}, {"params": ps[1::2], "weight_decay": 0.0}]  # wd 0.05 and 0.0, different lr (set_lr)
    opt = FusedAdamW(groups, lr=lr_at(0), betas=BETAS, eps=EPS, weight_decay=WD, capturable=capturable)
    return ps, opt, LossScaler(init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL)


def grads_of(k):
    """the (loss-scaled) gradients of step k, seeded; None for the last tensor; one inf at step INF_STEP"""
    g = torch.Generator().manual_seed(100 + k)
    # (0.05: the unscaled norm is ~7 at the initial scale, clipped at 5, and ~3.6, unclipped, once the scale has doubled)
    out = [torch.randn(n, generator=g) * (0.05 * INIT_SCALE) for n in numels()[:-1]]
    if k == INF_STEP:
        out[4][numels()[4] - 1] = float("inf")
    return [t.to(dev()) for t in out] + [None]


def snapshot(ps, opt, scaler, norm):
    torch.cuda.synchronize()
    return {"params": [p.detach().clone() for p in ps], "m": opt._exp_avg.clone(), "v": opt._exp_avg_sq.clone(),
            "ctrl": opt._ctrl.clone(), "norm": norm.clone(), "scale": scaler._scale.clone(),
            "tracker": scaler._growth_tracker.clone()}


def assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got["params"], want["params"])):
        assert same(a, b), f"{what}: parameter {i}"
    for k in ("m", "v", "ctrl", "norm", "scale", "tracker"):
        assert same(got[k], want[k]), f"{what}: {k} {got[k].flatten()[:8].tolist()} vs {want[k].flatten()[:8].tolist()}"


@pytest.fixture(scope="module")
def by_value():
    """STEPS + EXTRA eager steps of the by-value path (capturable=False): the reference, computed once"""
    ps, opt, scaler = make(False)
    snaps = []
    for k in range(STEPS + EXTRA):
        set_lr(opt, k)
        for p, g in zip(ps, grads_of(k)):
            p.grad = g
        snaps.append(snapshot(ps, opt, scaler, opt.clip_and_step(5.0, scaler)))
    # the reference itself behaves as the issue says: step 3 is skipped, the scale backs off, the counter stays
    assert snaps[INF_STEP]["ctrl"][1].item() == 1.0 and snaps[INF_STEP]["ctrl"][4].item() == snaps[INF_STEP - 1]["ctrl"][4].item() == 2.0
    assert snaps[INF_STEP]["scale"].item() == 0.5 * snaps[INF_STEP - 1]["scale"].item()
    for a, b in zip(snaps[INF_STEP]["params"], snaps[INF_STEP - 1]["params"]):
        assert same(a, b)
    assert snaps[1]["scale"].item() == 2.0 * INIT_SCALE  # (two good steps: the scale grew once)
    assert snaps[-1]["ctrl"][4].item() == STEPS + EXTRA - 1 and all(torch.isfinite(p).all() for p in snaps[-1]["params"])
    assert ps[-1] not in opt.state and same(snaps[-1]["params"][-1], snaps[0]["params"][-1])
    return snaps


def test_by_value_equals_by_device(by_value):
    """1. capturable=True, eager, against capturable=False: bit for bit after every step -- parameters, both state buffers, the
    control block, the norm, the scaler's scale and tracker -- with lr moving every step and step 3 skipped on both"""
    ps, opt, scaler = make(True)
    assert opt.param_groups[0]["capturable"] is True and opt.defaults["capturable"] is True
    for k in range(STEPS):
        set_lr(opt, k)
        for p, g in zip(ps, grads_of(k)):
            p.grad = g
        assert_same(snapshot(ps, opt, scaler, opt.clip_and_step(5.0, scaler)), by_value[k], f"eager step {k + 1}")
    assert opt.push_hyperparameters() is False  # nothing changed since the last step uploaded them


def test_replay_follows_the_learning_rate(by_value):
    """2. ONE captured clip_and_step(5.0, scaler), gradients in static buffers, replayed with the lr sequence and the inf step of
    case 1 (push_hyperparameters() between replays): bit-identical to the eager by-value run after every replay, and after two
    more replays with param_groups untouched.  A graph with the hyper-parameters baked in fails at the second replay."""
    ps, opt, scaler = make(True)
    init = [p.detach().clone() for p in ps]
    for p in ps[:-1]:
        p.grad = torch.zeros_like(p)  # static: allocated once, filled by copy_ before each replay

    def fill(k):
        for p, g in zip(ps[:-1], grads_of(k)):
            p.grad.copy_(g)

    set_lr(opt, 0)
    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the usual warm-up off the capture stream (it also pushes the hyper-parameters)
        opt.clip_and_step(5.0, scaler)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():  # back to the initial state, in the same buffers
        for p, q in zip(ps, init):
            p.copy_(q)
        opt._exp_avg.zero_()
        opt._exp_avg_sq.zero_()
        opt._ctrl.zero_()
        scaler._scale.fill_(INIT_SCALE)
        scaler._growth_tracker.fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = opt.clip_and_step(5.0, scaler)
    assert ps[-1] not in opt.state and all(p in opt.state for p in ps[:-1])  # state entries: exactly the tensors with a gradient
    versions = [p._version for p in ps]
    for k in range(STEPS + EXTRA):
        if k < STEPS:
            set_lr(opt, k)
        fill(k)
        assert opt.push_hyperparameters() is (0 < k < STEPS)  # uploads only on change (step 1's values: the warm-up pushed them)
        graph.replay()
        opt.bump_versions()
        assert_same(snapshot(ps, opt, scaler, norm), by_value[k], f"replay {k + 1}")
    assert [p._version for p in ps[:-1]] == [v + STEPS + EXTRA for v in versions[:-1]] and ps[-1]._version == versions[-1]


def test_bad_hyperparameters_skip_the_step():
    """3. lr = -1 on the device (the by-value entry rejects it on the host; a kernel cannot return an error): found_inf is set, the
    step is skipped -- parameters, state and the counter bitwise unchanged -- and the norm is nan; the next good step runs"""
    ps, opt, scaler = make(True)

    def step(k):
        for p, g in zip(ps, grads_of(k)):
            p.grad = g
        return snapshot(ps, opt, scaler, opt.clip_and_step(5.0, scaler))

    good = step(0)
    assert good["ctrl"][4].item() == 1.0 and torch.isfinite(good["norm"])
    opt.param_groups[0]["lr"] = -1.0
    assert opt.push_hyperparameters() is True
    bad = step(1)
    assert torch.isnan(bad["norm"]) and torch.isnan(bad["ctrl"][0]) and bad["ctrl"][1].item() == 1.0
    assert bad["ctrl"][4].item() == 1.0
    for a, b in zip(bad["params"], good["params"]):
        assert same(a, b)
    assert same(bad["m"], good["m"]) and same(bad["v"], good["v"])
    assert bad["scale"].item() == 0.5 * good["scale"].item()  # found_inf: the scaler backs off as for an inf gradient
    set_lr(opt, 1)
    again = step(1)
    assert again["ctrl"][4].item() == 2.0 and torch.isfinite(again["norm"]) and again["ctrl"][1].item() == 0.0
    assert not same(again["params"][3], good["params"][3]) and all(torch.isfinite(p).all() for p in again["params"])


def test_whole_step_graphed_with_scaler():
    """4. the whole fp16 train step with the LossScaler and FusedAdamW captured (the model, batch and criterion of
    test_gpu_models.test_graphed_train_step_replays_the_eager_step): four replays with an lr that changes every step against four
    eager train_step(loss_scaler=...) calls from the same state with the same dropout seeds and offsets.  Criterion, copied from
    that test: losses (and here the gradient norms) within 2e-3 relative, cosine of the accumulated updates >= 0.98 (hipBLASLt
    may pick another algorithm for the heads' GEMMs while capturing, so not bit-equal).  Then eval: a forward of the replayed
    model equals that of a fresh model loaded from its state_dict, i.e. bump_versions() reached the weight caches."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW, LossScaler
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=17, device=dev())
    lrs = [1e-3 * f for f in (0.25, 0.5, 1.0, 0.8)]
    kw = dict(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4)
    out = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(**kw).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        assert isinstance(opt, FusedAdamW)
        scaler = LossScaler(init_scale=2.0 ** 10)
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16, loss_scaler=scaler)
            assert gs.graphed is True and gs.why == "", gs.why
            drawn = Fn._seed_counter  # two warm-up steps and the capture drew the layers' dropout seeds: three equal shares
            assert drawn > 0 and drawn % 3 == 0
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses, norms = [], []
            for lr in lrs:
                for g in opt.param_groups:
                    g["lr"] = lr
                if use_graph:
                    loss, norm = gs(), gs.grad_norm
                else:  # the eager step, drawing the seeds the capture drew and walking the same device offset
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                    loss, norm = H.train_step(model, crit, opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler)
                losses.append(loss.clone())
                norms.append(norm.clone())
            torch.cuda.synchronize()
            out.append((losses, {n: (p.detach() - start[n]).double() for n, p in model.named_parameters() if n in start}, norms))
            if use_graph:
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
    for a, b in zip(out[0][0], out[1][0]):
        print("loss", a.item(), b.item())
        assert abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    for a, b in zip(out[0][2], out[1][2]):
        print("grad norm", a.item(), b.item())
        assert math.isfinite(a.item()) and abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    num = sum((out[0][1][n] * out[1][1][n]).sum().item() for n in out[0][1])
    den = (sum((out[0][1][n] ** 2).sum().item() for n in out[0][1]) * sum((out[1][1][n] ** 2).sum().item() for n in out[1][1])) ** 0.5
    print("cosine", num / den)
    assert num / den >= 0.98, num / den


def test_non_capturable_optimizer_is_refused():
    """5. a by-value FusedAdamW cannot follow param_groups inside a graph: TypeError naming capturable=True, not an eager fallback"""
    from mtlora_amd import mtl_harness as H
    ps, opt, scaler = make(False)
    with pytest.raises(TypeError, match="capturable=True"):
        H.GraphedTrainStep(None, None, opt, torch.zeros(1, device=dev()), {}, loss_scaler=scaler)
