"""FusedSGD and FusedLAMB on the GPU (mtlora_amd/optim.py, csrc/optim.hip: mtlora_sgd_update[_dev], mtlora_lamb_update[_dev]).

The tensor set, the fp64 references (torch.optim.SGD + clip_grad_norm_ in fp64; optim.lamb_update_torch in fp64) and the error
measures are tests/test_cpu_optim_sgd_lamb.py's.  As in tests/test_gpu_optim.py what is compared is the UPDATE delta, never p.

Bounds: the project's (tests/test_gpu_optim.py)
    norm    1e-5 relative
    state   1e-5 of max|ref|, per tensor
    update  max|delta - delta_ref| <= 2e-4 max|delta_ref| + ulp_fp32(max|p|), per tensor
unless the fp32 stand-in for the kernel (torch.optim.SGD in fp32; lamb_update_torch in fp32) measured on these exact inputs on the
CPU shows more than a quarter of one of them; that bound is then 4 x the stand-in's figure (the margin covers the kernels' other
reduction order and FMA contraction).  The stand-in figures (test_cpu_optim_sgd_lamb.test_fp32_standins_against_fp64, which also
asserts that BOUNDS below is what this rule gives; recorded in profiles/optim_sgd_lamb_tests.txt):
    SGD   norm 1.2e-7   state 1.2e-7   update 0 beyond the ulp term         -> the project's bounds
    LAMB  norm 4.7e-8   state 2.2e-7   update 8.5e-9 beyond the ulp term    -> the project's bounds
(LAMB's "moved by lr |p|" check uses the update's relative bound: |p| and |u| are fp32 sums, each within the norm bound.)
No bound was derived from the kernels' output.  The measured figures are printed, and appended to the file named by
MTLORA_OPTIM_FIGURES when that is set."""
import numpy as np
import pytest
import torch

from test_cpu_optim_sgd_lamb import (BETAS, GRAD_SCALES, LAMB_EPS, LR, MAX_GRAD_NORM, MAX_NORM, MOMENTUM, SHAPES, WD, ZERO_SHAPE, TorchLAMB,
                                     TorchSGD, check_delta, common_inputs, decays, groups_of, norm_figure, snap, state_figure, write_figures)

pytestmark = pytest.mark.gpu

BOUNDS = {"sgd": {"norm": 1e-5, "state": 1e-5, "delta": 2e-4}, "lamb": {"norm": 1e-5, "state": 1e-5, "delta": 2e-4}}
LAMB_SHAPES = SHAPES + [ZERO_SHAPE]
_FIGURES = []


def dev():
    return torch.device("cuda:0")


def fig(what, value):
    _FIGURES.append(f"{what}: {value:.3e}")
    print(_FIGURES[-1])


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    write_figures(_FIGURES)


def make(alg, init, shapes=None, capturable=False, **kw):
    from mtlora_amd.optim import FusedLAMB, FusedSGD
    shapes = shapes or (SHAPES if alg == "sgd" else LAMB_SHAPES)
    ps = [torch.nn.Parameter(t.to(dev())) for t in init]
    if alg == "sgd":
        kw = {"momentum": MOMENTUM, "nesterov": True, **kw}
        return ps, FusedSGD(groups_of(ps, shapes), lr=LR, weight_decay=WD, capturable=capturable, **kw)
    return ps, FusedLAMB(groups_of(ps, shapes), lr=LR, betas=BETAS, eps=LAMB_EPS, weight_decay=WD, max_grad_norm=MAX_GRAD_NORM,
                         capturable=capturable, **kw)


def make_ref(alg, init, shapes=None):
    return TorchSGD(init, shapes or SHAPES) if alg == "sgd" else TorchLAMB(init, shapes or LAMB_SHAPES)


def inputs(alg, **kw):
    return common_inputs(**kw) if alg == "sgd" else common_inputs(LAMB_SHAPES, zero=(ZERO_SHAPE,), **kw)


KEYS = {"sgd": ("momentum_buffer",), "lamb": ("exp_avg", "exp_avg_sq")}


def set_grads(ps, grads, mult=1.0):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else (g * mult).to(dev())


def check_norm(what, alg, got, ref):
    err = norm_figure(got.double().item(), ref)
    fig(f"{what}: norm relative error", err)
    assert got.ndim == 0 and got.is_cuda and err <= BOUNDS[alg]["norm"], (what, got.item(), float(ref))


def check_state(what, alg, opt, ps, ref):
    worst = 0.0
    for i, p in enumerate(ps):
        for k in KEYS[alg]:
            r = ref.state(i, k)
            if r is None:
                assert p not in opt.state or opt.state[p][k] is None, (what, i)
                continue
            got = opt.state[p][k]
            assert got.shape == r.shape
            err = state_figure(got, r)
            worst = max(worst, err)
            assert err <= BOUNDS[alg]["state"], (what, i, k, err)
    fig(f"{what}: max state error / max|ref|", worst)


def bits(ps, opt):
    torch.cuda.synchronize()
    return [p.detach().clone() for p in ps] + [opt._exp_avg.clone(), opt._exp_avg_sq.clone(), opt._ctrl[4].clone()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_clip_and_step_vs_fp64(alg):
    """1 / 2. three clip_and_step calls (gradient scales 1e-7, 0.01, 30: max_norm idle, idle, active; LAMB's max_grad_norm idle,
    active, active) against the fp64 reference: norm, update and state after every step, the step count; LAMB: the decay group moved
    by lr |p| per tensor and the no-decay group did not; step() alone; three runs are bit-equal."""
    init, grads = inputs(alg)
    shapes = SHAPES if alg == "sgd" else LAMB_SHAPES
    ref = make_ref(alg, init)

    def run(check):
        ps, opt = make(alg, init)
        for k, gs in enumerate(grads):
            before = snap(ps)
            set_grads(ps, gs)
            norm = opt.clip_and_step(MAX_NORM)
            if not check:
                continue
            rb = snap(ref.ps)
            rnorm = ref.step(gs)
            what = f"{alg} step {k + 1} (gradients x {GRAD_SCALES[k]:g})"
            check_norm(what, alg, norm, rnorm)
            assert (float(rnorm) > MAX_NORM) == (k == 2)
            after = snap(ps)
            check_delta(what, before, after, rb, snap(ref.ps), BOUNDS[alg]["delta"])
            check_state(what, alg, opt, ps, ref)
            if alg == "sgd":
                assert "step" not in opt.state[ps[0]] and set(opt.state[ps[0]]) == {"momentum_buffer"}
                continue
            assert opt.state[ps[0]]["step"].item() == k + 1 == ref.st["step"]
            c = opt._ctrl[7].item()  # LAMB's own clip: idle in step 1, active in steps 2 and 3
            assert (c == 1.0) == (k == 0) and abs(c - ref.last["clip"].item()) <= BOUNDS[alg]["norm"] * c
            for i, s in enumerate(shapes):
                if int(np.prod(s)) == 1 or (s == ZERO_SHAPE and k == 0):
                    continue
                moved, trust = (after[i] - before[i]).norm().item(), LR * before[i].norm().item()
                if decays(s):  # |delta p| = ratio |u| = lr |p|
                    assert abs(moved - trust) <= BOUNDS[alg]["delta"] * trust, (k, i, moved, trust)
                else:  # ratio = lr: the trust ratio would have moved it by lr |p|, far outside the bound
                    assert abs(moved - trust) > 10 * BOUNDS[alg]["delta"] * trust, (k, i, moved, trust)
        return bits(ps, opt)

    first = run(True)
    for _ in range(2):  # fixed-order reductions: bit-reproducible
        assert same(first, run(False))

    # step() alone: no clip, although the norm (~4.8e3) is far above any max_norm
    ps, opt = make(alg, init)
    ref = make_ref(alg, init)
    before, rb = snap(ps), snap(ref.ps)
    set_grads(ps, grads[2])
    assert opt.step() is None
    ref.step(grads[2], max_norm=None)
    check_delta(f"{alg} step() without clip", before, snap(ps), rb, snap(ref.ps), BOUNDS[alg]["delta"])
    check_state(f"{alg} step() without clip", alg, opt, ps, ref)


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_misaligned_views_and_missing_grads(alg):
    """3. a parameter and a gradient that start one element into a larger buffer (the scalar paths), a parameter whose gradient is
    None in step 2 only and one that never gets a gradient: bitwise unchanged, no state entry, no version bump"""
    shapes = [(5000,), (4099,), (1023,), (300,), (2, 4096)]  # A: misaligned parameter; B: misaligned gradient; C; D: never; E
    init, grads = common_inputs(shapes, seed=1)
    A, B, C, D = 0, 1, 2, 3
    bufA = torch.zeros(shapes[A][0] + 1, device=dev())
    bufA[1:].copy_(init[A])
    ps = [torch.nn.Parameter(bufA[1:] if i == A else t.to(dev())) for i, t in enumerate(init)]
    assert ps[A].data_ptr() % 16 == 4 and ps[A].is_contiguous()
    from mtlora_amd.optim import FusedLAMB, FusedSGD
    opt = (FusedSGD(groups_of(ps, shapes), lr=LR, momentum=MOMENTUM, nesterov=True, weight_decay=WD) if alg == "sgd" else
           FusedLAMB(groups_of(ps, shapes), lr=LR, betas=BETAS, eps=LAMB_EPS, weight_decay=WD, max_grad_norm=MAX_GRAD_NORM))
    ref = make_ref(alg, init, shapes)
    for k in range(3):
        gs = list(grads[k])
        gs[D] = None
        if k == 1:
            gs[C] = None
        set_grads(ps, gs)
        gbuf = torch.zeros(shapes[B][0] + 1, device=dev())
        gbuf[1:].copy_(gs[B])
        ps[B].grad = gbuf[1:]
        assert ps[B].grad.data_ptr() % 16 == 4
        before, rb = snap(ps), snap(ref.ps)
        vers = [p._version for p in ps]
        c_bits = ps[C].detach().clone()
        norm = opt.clip_and_step(MAX_NORM)
        rnorm = ref.step(gs)
        what = f"{alg} misaligned / missing step {k + 1}"
        check_norm(what, alg, norm, rnorm)
        check_delta(what, before, snap(ps), rb, snap(ref.ps), BOUNDS[alg]["delta"])
        check_state(what, alg, opt, ps, ref)
        assert ps[D]._version == vers[D] and torch.equal(ps[D].detach().cpu(), init[D]) and ps[D] not in opt.state
        assert all(p._version > v for i, (p, v) in enumerate(zip(ps, vers)) if gs[i] is not None)
        if k == 1:
            assert ps[C]._version == vers[C] and torch.equal(ps[C].detach(), c_bits)
        assert bufA[0].item() == 0.0  # nothing was written in front of the misaligned parameter
    o = opt._offsets[next(i for i, p in enumerate(opt._params) if p is ps[D])]  # its slice of the flat state buffers
    assert not opt._exp_avg[o:o + shapes[D][0]].any() and not opt._exp_avg_sq[o:o + shapes[D][0]].any()


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_loss_scaler_skip_backoff_growth(alg):
    """4. LossScaler(init_scale=1024, growth_interval=2), gradients pre-multiplied by the scale: a good step, a step with one inf
    (skipped on the device: parameters, state buffers and the counter bitwise unchanged, scale 512, tracker 0), two good steps
    (the scale grows back to 1024)"""
    from mtlora_amd.optim import LossScaler
    init, _ = inputs(alg)
    _, grads = inputs(alg, scales=(0.01, 0.01, 30.0, 0.01), seed=2)
    ps, opt = make(alg, init)
    ref = make_ref(alg, init)
    scaler = LossScaler(init_scale=1024.0, growth_interval=2)
    expect = [(1024.0, 1), (512.0, 0), (512.0, 1), (1024.0, 0)]  # (scale, tracker) after each call
    for k, gs in enumerate(grads):
        scale = scaler.get_scale()
        set_grads(ps, gs, mult=scale)
        before, rb = snap(ps), snap(ref.ps)
        what = f"{alg} loss scaler call {k + 1} (scale {scale:g})"
        if k == 1:
            ps[5].grad[1234] = float("inf")
            keep = bits(ps, opt)
            norm = opt.clip_and_step(MAX_NORM, scaler)
            assert not torch.isfinite(norm).item()
            assert same(keep, bits(ps, opt)) and opt._ctrl[4].item() == 1
        else:
            norm = opt.clip_and_step(MAX_NORM, scaler)
            rnorm = ref.step(gs)
            check_norm(what, alg, norm, rnorm)
            check_delta(what, before, snap(ps), rb, snap(ref.ps), BOUNDS[alg]["delta"])
            check_state(what, alg, opt, ps, ref)
        sd = scaler.state_dict()
        assert (sd["scale"], sd["_growth_tracker"]) == expect[k], (k, sd)
    assert opt._ctrl[4].item() == 3
    if alg == "lamb":
        assert opt.state[ps[0]]["step"].item() == 3


def test_sgd_state_dict_interchanges_with_torch_sgd():
    """5. a checkpoint written by either optimizer loads into the other: same keys, and both continue alike"""
    from mtlora_amd.optim import FusedSGD
    init, _ = common_inputs()
    _, grads = common_inputs(scales=(0.01, 30.0, 0.01, 30.0), seed=4)
    ps, opt = make("sgd", init)
    for k in range(2):
        set_grads(ps, grads[k])
        opt.clip_and_step(MAX_NORM)
    sd = opt.state_dict()

    def torch_twin(src):
        qs = [torch.nn.Parameter(p.detach().clone()) for p in src]
        return qs, torch.optim.SGD(groups_of(qs), lr=LR, momentum=MOMENTUM, nesterov=True, weight_decay=WD, foreach=False)

    tps, topt = torch_twin(ps)
    native = topt.state_dict()
    topt.load_state_dict(sd)

    def both_step(k, hip_ps, hip_opt, what):
        before, tb = snap(hip_ps), snap(tps)
        set_grads(hip_ps, grads[k])
        set_grads(tps, grads[k])
        norm = hip_opt.clip_and_step(MAX_NORM)
        tnorm = torch.nn.utils.clip_grad_norm_(tps, MAX_NORM)
        topt.step()
        check_norm(what, "sgd", norm, tnorm.double().cpu())
        check_delta(what, before, snap(hip_ps), tb, snap(tps), BOUNDS["sgd"]["delta"])
        for p, q in zip(hip_ps, tps):
            assert state_figure(hip_opt.state[p]["momentum_buffer"], topt.state[q]["momentum_buffer"].cpu()) <= BOUNDS["sgd"]["state"]

    both_step(2, ps, opt, "FusedSGD state into torch SGD, step 3")
    tsd = topt.state_dict()
    assert set(sd) == set(tsd) == set(native)
    assert all(set(a) == set(b) for a, b in zip(sd["param_groups"], native["param_groups"]))
    assert set(sd["state"]) == set(tsd["state"]) and all(set(sd["state"][i]) == set(tsd["state"][i]) == {"momentum_buffer"} for i in sd["state"])
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in tps]
    opt2 = FusedSGD(groups_of(ps2), lr=LR, momentum=MOMENTUM, nesterov=True, weight_decay=WD)
    opt2.load_state_dict(tsd)
    both_step(3, ps2, opt2, "torch SGD state into FusedSGD, step 4")


def test_lamb_state_dict_reload_continues_bit_equal():
    """5. FusedLAMB's state (FusedAdamW's layout, LAMB's group keys) into a fresh FusedLAMB: the continuation is bit-equal to the
    uninterrupted run"""
    init, grads = inputs("lamb", scales=(0.01, 30.0, 0.01, 1e-7), seed=4)
    ps, opt = make("lamb", init)
    for k in range(2):
        set_grads(ps, grads[k])
        opt.clip_and_step(MAX_NORM)
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"].item() == 2
    assert {"lr", "betas", "eps", "weight_decay", "max_grad_norm", "use_nvlamb", "bias_correction"} <= set(sd["param_groups"][0])
    ps2, opt2 = make("lamb", [p.detach().cpu() for p in ps])
    opt2.load_state_dict(sd)
    for k in (2, 3):
        for q, o in ((ps, opt), (ps2, opt2)):
            set_grads(q, grads[k])
            o.clip_and_step(MAX_NORM)
    assert same(bits(ps, opt), bits(ps2, opt2))
    sd["state"][0]["step"] = sd["state"][0]["step"] + 1
    with pytest.raises(ValueError, match="FusedLAMB keeps one step counter"):
        opt2.load_state_dict(sd)


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_capturable_is_bit_identical_and_follows_param_groups(alg):
    """6. the _dev entry (hyper-parameters in device memory) against the by-value entry, bit for bit; then one clip_and_step captured
    in torch.cuda.graph and replayed three times with the lr changed between replays (push_hyperparameters), bit-equal to the eager
    by-value sequence"""
    from mtlora_amd.optim import LossScaler
    init, grads = inputs(alg)
    lrs = [LR, 0.5 * LR, 0.25 * LR, 2.0 * LR]

    def eager(capturable):
        ps, opt = make(alg, init, capturable=capturable)
        sc = LossScaler(init_scale=4.0)
        for k, lr in enumerate(lrs):
            for g in opt.param_groups:
                g["lr"] = lr
            set_grads(ps, grads[k % 3], mult=sc.get_scale())
            opt.clip_and_step(MAX_NORM, sc)
        return bits(ps, opt)

    want = eager(False)
    assert same(want, eager(True))

    ps, opt = make(alg, init, capturable=True)
    sc = LossScaler(init_scale=4.0)
    static = [torch.zeros_like(p) for p in ps]
    for p, s in zip(ps, static):
        p.grad = s
    for s, g in zip(static, grads[0]):
        s.copy_(g * 4.0)
    opt.clip_and_step(MAX_NORM, sc)  # step 1 eagerly (initialises the scaler and the state entries)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            norm = opt.clip_and_step(MAX_NORM, sc)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        for s, g in zip(static, grads[k % 3]):
            s.copy_(g * 4.0)
        opt.push_hyperparameters()
        vers = ps[0]._version
        graph.replay()
        opt.bump_versions()
        assert ps[0]._version > vers
    assert torch.isfinite(norm).item()
    assert same(want, bits(ps, opt))


def test_train_step_and_graphed_train_step():
    """7. two train steps with build_optimizer(name="sgd", impl="hip") against impl="torch" on the same GPU gradients, to the AdamW
    train-step test's bound; two steps of name="lamb" eager (train_step with a LossScaler) against GraphedTrainStep(loss_scaler=),
    bit-equal"""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedLAMB, FusedSGD, LossScaler
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=13, device=dev())

    def fresh(name, impl, capturable=False):
        torch.manual_seed(5)
        Fn._seed_counter = 0
        Fn.droppath_reset()
        model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, seed=3).to(dev()).train()
        return model, H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl=impl, name=name, capturable=capturable)

    def named(model):
        return {n: p.detach().double().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}

    out = {}
    for impl in ("torch", "hip"):
        model, crit, opt = fresh("sgd", impl)
        assert isinstance(opt, FusedSGD if impl == "hip" else torch.optim.SGD)
        steps = []
        for _ in range(2):
            before = named(model)
            loss, norm = H.train_step(model, crit, opt, img, tg)
            steps.append((loss.clone(), norm.clone(), before, named(model)))
        out[impl] = steps
    for k in range(2):
        h, t = out["hip"][k], out["torch"][k]
        names = list(h[2])
        if k == 0:
            assert torch.equal(h[0], t[0]) and all(torch.equal(h[2][n], t[2][n]) for n in names)
        check_norm(f"train_step sgd step {k + 1}: norm against clip_grad_norm_ (fp32, GPU)", "sgd", h[1], t[1].double().cpu())
        # (each implementation's own delta: from step 2 on the two start from parameters that differ by step 1's rounding)
        check_delta(f"train_step sgd step {k + 1} against torch SGD", [h[2][n] for n in names], [h[3][n] for n in names],
                    [t[2][n] for n in names], [t[3][n] for n in names], BOUNDS["sgd"]["delta"], names)

    # LAMB: two replays against two eager train_step calls from the same state, with the dropout seeds and the device seed offset
    # the capture drew (the choreography of test_gpu_optim_capturable.test_whole_step_graphed_with_scaler); bit-equal
    kw = dict(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4)
    ends = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(**kw).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", name="lamb", capturable=True)
        assert isinstance(opt, FusedLAMB)
        scaler = LossScaler(init_scale=2.0 ** 10)
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16, loss_scaler=scaler)
            assert gs.graphed is True and gs.why == "", gs.why
            drawn = Fn._seed_counter
            assert drawn > 0 and drawn % 3 == 0
            for _ in range(2):
                if use_graph:
                    gs()
                else:
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                    H.train_step(model, crit, opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler)
            torch.cuda.synchronize()
            ends.append((named(model), opt._exp_avg.clone(), opt._exp_avg_sq.clone(), opt._ctrl[4].item(), scaler.get_scale()))
        finally:
            Fn.set_seed_offset(None)
    worst = max((ends[0][0][n] - ends[1][0][n]).abs().max().item() for n in ends[0][0])
    fig("lamb: graphed against eager after two steps, max |p - p'|", worst)
    assert ends[0][3] == ends[1][3] and ends[0][4] == ends[1][4]
    assert all(torch.equal(ends[0][0][n], ends[1][0][n]) for n in ends[0][0])
    assert torch.equal(ends[0][1], ends[1][1]) and torch.equal(ends[0][2], ends[1][2])


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_snapshot_round_trip(alg):
    """8. TrainState snapshot -> more steps -> restore() -> the same steps again: bit-equal to the uninterrupted run"""
    from mtlora_amd.checkpoint import TrainState
    from mtlora_amd.optim import LossScaler
    init, grads = inputs(alg, scales=(0.01, 30.0, 0.01, 1e-7), seed=6)
    shapes = SHAPES if alg == "sgd" else LAMB_SHAPES

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList(ps)

    ps, opt = make(alg, init, shapes, capturable=True)
    model, sc = Holder(ps), LossScaler(init_scale=8.0, growth_interval=2)
    state = TrainState(model, opt, None, sc)

    def go(ks):
        for k in ks:
            set_grads(ps, grads[k], mult=sc.get_scale())
            opt.clip_and_step(MAX_NORM, sc)

    go((0, 1))
    handle = state.snapshot()
    st = handle.state(copy=True)
    go((2, 3))
    want = bits(ps, opt) + [sc._scale.clone()]
    assert set(st["optimizer"]["state"][0]) == ({"momentum_buffer"} if alg == "sgd" else {"step", "exp_avg", "exp_avg_sq"})
    state.restore(st)
    go((2, 3))
    got = bits(ps, opt) + [sc._scale.clone()]
    if alg == "sgd":  # (SGD's state has no step entry: the device counter restarts, and nothing reads it)
        want, got = want[:-2] + want[-1:], got[:-2] + got[-1:]
    assert same(want, got)


@pytest.mark.parametrize("alg", ["sgd", "lamb"])
def test_out_of_scope_combinations_raise(alg):
    """9. accumulation inside the update and the device-side schedule are FusedAdamW's: TypeError naming the class"""
    from mtlora_amd import lr_scheduler as S
    from mtlora_amd import mtl_harness as H
    init, grads = inputs(alg)
    ps, opt = make(alg, init, capturable=True)
    name = type(opt).__name__
    set_grads(ps, grads[1])
    keep = bits(ps, opt)
    with pytest.raises(TypeError, match=name):
        opt.clip_and_step(MAX_NORM, None, accumulation_steps=2)
    with pytest.raises(TypeError, match=name):
        opt.prepare_accumulation()
    sched = S.StepLRScheduler(opt, decay_t=10, decay_rate=0.5, t_in_epochs=False)
    with pytest.raises(TypeError, match=name):
        opt.attach_schedule(sched)
    for kw in (dict(accumulation_steps=2), dict(lr_scheduler=sched)):
        with pytest.raises(TypeError, match=name):
            H.GraphedTrainStep(None, None, opt, torch.zeros(1, device=dev()), {}, **kw)
    assert same(keep, bits(ps, opt))
