"""The fused gradient clip + loss scaler + AdamW update on the GPU (mtlora_amd/optim.py, csrc/optim.hip).

Every expected value is an fp64 restatement on the CPU: ``torch.optim.AdamW`` and ``clip_grad_norm_`` on float64 copies (cases 5
and 6 compare with torch's fp32 AdamW on the GPU, the path ``build_optimizer(impl="torch")`` takes).  What is compared is always
the UPDATE delta = p_after - p_before, never p: at p ~ 1 a missing weight decay (5 % of delta) or bias correction would vanish
inside any tolerance on p.

Bounds (fp32 AdamW standing in for the kernel measures 1.4e-7 on the norm, 3.8e-7 on the state and 3.1e-5 max|delta_ref| on the
update -- the half-ulp of storing p ~ 1 in fp32 against a step of about lr):
    norm    1e-5 relative (the project's float-sum bound, test_gpu_eval.FLOAT_RTOL)
    state   1e-5 of max|ref|, per tensor
    update  max|delta - delta_ref| <= 2e-4 max|delta_ref| + ulp_fp32(max|p|), per tensor
The measured figures are printed, and appended to the file named by MTLORA_OPTIM_FIGURES when that is set (profiles/optim_gpu_tests.txt
is where such a run belongs)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NORM_RTOL = 1e-5
STATE_RTOL = 1e-5
DELTA_RTOL = 2e-4
SHAPES = [(1,), (3,), (64,), (1023,), (4096,), (4097,), (3 * 4096 + 5,), (37, 129)]
LR, BETAS, EPS, WD, MAX_NORM = 1e-2, (0.9, 0.999), 1e-8, 0.05, 5.0
GRAD_SCALES = (1e-7, 0.01, 30.0)  # eps carries ~10 % of the first denominator; clip idle (norm ~1.6); clip active (norm ~4.8e3)

_FIGURES = []


def dev():
    return torch.device("cuda:0")


def fig(what, value):
    _FIGURES.append(f"{what}: {value:.3e}")
    print(_FIGURES[-1])


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("MTLORA_OPTIM_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(_FIGURES) + "\n")


def decays(shape):
    n = int(np.prod(shape))
    return n >= 4096 or len(shape) == 2


def common_inputs(shapes=SHAPES, scales=GRAD_SCALES, seed=0):
    """(initial values, per-step gradients): fp32 CPU tensors from one seeded generator"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * sc for s in shapes] for sc in scales]
    return init, grads


def groups_of(params, shapes=SHAPES):
    return [{"params": [p for p, s in zip(params, shapes) if decays(s)]},
            {"params": [p for p, s in zip(params, shapes) if not decays(s)], "weight_decay": 0.0}]


def make_hip(init, shapes=SHAPES):
    from mtlora_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(t.to(dev())) for t in init]
    return ps, FusedAdamW(groups_of(ps, shapes), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)


def make_ref(init, shapes=SHAPES):
    ps = [torch.nn.Parameter(t.double()) for t in init]
    return ps, torch.optim.AdamW(groups_of(ps, shapes), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)


def ref_step(ps, opt, grads, max_norm=MAX_NORM):
    """one reference step on the fp64 copies; a None gradient leaves that parameter out, as torch does.  Returns the norm."""
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.double().clone()
    live = [p for p in ps if p.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False) if max_norm else None
    opt.step()
    return norm


def snap(ps):
    return [p.detach().double().cpu().clone() for p in ps]


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def check_delta(what, before, after, ref_before, ref_after, names=None):
    worst = 0.0
    for i, (b, a, rb, ra) in enumerate(zip(before, after, ref_before, ref_after)):
        d, dr = a - b, ra - rb
        err, scale = (d - dr).abs().max().item(), dr.abs().max().item()
        bound = DELTA_RTOL * scale + ulp32(max(a.abs().max().item(), b.abs().max().item()))
        worst = max(worst, err / scale if scale > 0 else 0.0)
        assert err <= bound, (what, names[i] if names else i, err, bound, scale)
    fig(f"{what}: max |delta - delta_ref| / max|delta_ref|", worst)


def check_state(what, opt, ps, ref_opt, ref_ps):
    worst = 0.0
    for i, (p, rp) in enumerate(zip(ps, ref_ps)):
        if rp not in ref_opt.state:
            assert p not in opt.state, (what, i)
            continue
        for k in ("exp_avg", "exp_avg_sq"):
            got, ref = opt.state[p][k].double().cpu(), ref_opt.state[rp][k]
            assert got.shape == ref.shape
            err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
            worst = max(worst, err / scale)
            assert err <= STATE_RTOL * scale, (what, i, k, err, scale)
    fig(f"{what}: max state error / max|ref|", worst)


def check_norm(what, got, ref):
    err = abs(got.double().item() - ref.item()) / ref.item()
    fig(f"{what}: norm relative error", err)
    assert got.ndim == 0 and got.is_cuda and err <= NORM_RTOL, (what, got.item(), ref.item())


def set_grads(ps, grads, mult=1.0):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else (g * mult).to(dev())


def test_clip_adamw_vs_fp64():
    """three clip_and_step calls (gradient scales 1e-7, 0.01, 30) against fp64 clip_grad_norm_ + AdamW: norm, update, exp_avg,
    exp_avg_sq after every step; no decay where the group has none; step() alone (no clip); three runs are bit-equal."""
    init, grads = common_inputs()
    rps, ropt = make_ref(init)

    def run(check):
        ps, opt = make_hip(init)
        for k, gs in enumerate(grads):
            before = snap(ps)
            set_grads(ps, gs)
            norm = opt.clip_and_step(MAX_NORM)
            if check:
                rb = snap(rps)
                rnorm = ref_step(rps, ropt, gs)
                what = f"clip_adamw step {k + 1} (gradients x {GRAD_SCALES[k]:g})"
                check_norm(what, norm, rnorm)
                assert (rnorm.item() > MAX_NORM) == (k == 2)  # the clip is idle in steps 1 and 2 and active in step 3
                after = snap(ps)
                check_delta(what, before, after, rb, snap(rps))
                check_state(what, opt, ps, ropt, rps)
                assert opt.state[ps[0]]["step"].item() == k + 1
                if k == 1:  # no decay where the group has none: the decayed update is lr wd p away, far outside the bound
                    for i, s in enumerate(SHAPES):
                        if not decays(s) and int(np.prod(s)) > 1:
                            d = after[i] - before[i]
                            decayed = (rps[i].detach() - rb[i]) - LR * WD * rb[i]
                            assert (d - decayed).abs().max().item() > 10 * DELTA_RTOL * d.abs().max().item(), i
        torch.cuda.synchronize()
        return [p.detach().clone() for p in ps]

    first = run(True)
    for _ in range(2):  # fixed-order reductions: bit-reproducible
        again = run(False)
        assert all(torch.equal(a, b) for a, b in zip(first, again))

    # step() alone: plain AdamW, no clip, although the norm (~4.8e3) is far above any max_norm
    ps, opt = make_hip(init)
    rps, ropt = make_ref(init)
    before, rb = snap(ps), snap(rps)
    set_grads(ps, grads[2])
    assert opt.step() is None
    ref_step(rps, ropt, grads[2], max_norm=None)
    check_delta("step() without clip", before, snap(ps), rb, snap(rps))
    check_state("step() without clip", opt, ps, ropt, rps)


def test_misaligned_views_and_missing_grads():
    """a parameter and a gradient that start one element into a larger buffer (4-byte aligned only: the scalar paths), a parameter
    whose gradient is None in step 2 only, and one that never gets a gradient.

    FusedAdamW keeps ONE step counter (the issue's design), torch one per parameter: for the parameter that misses step 2 the
    reference's counter is advanced by hand in that step, so that its step 3 uses t = 3 as the kernels do."""
    from mtlora_amd.optim import FusedAdamW
    shapes = [(5000,), (4099,), (1023,), (300,), (2, 4096)]  # A: misaligned parameter; B: misaligned gradient; C; D: never; E
    init, grads = common_inputs(shapes, seed=1)
    A, B, C, D = 0, 1, 2, 3
    bufA = torch.zeros(shapes[A][0] + 1, device=dev())
    bufA[1:].copy_(init[A])
    ps = [torch.nn.Parameter(bufA[1:] if i == A else t.to(dev())) for i, t in enumerate(init)]
    assert ps[A].data_ptr() % 16 == 4 and ps[A].is_contiguous()
    opt = FusedAdamW(groups_of(ps, shapes), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    rps, ropt = make_ref(init, shapes)
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
        before, rb = snap(ps), snap(rps)
        vers = [p._version for p in ps]
        c_bits = ps[C].detach().clone()
        norm = opt.clip_and_step(MAX_NORM)
        rnorm = ref_step(rps, ropt, gs)
        if k == 1:
            ropt.state[rps[C]]["step"] += 1  # the single counter, see the docstring
        what = f"misaligned / missing step {k + 1}"
        check_norm(what, norm, rnorm)
        check_delta(what, before, snap(ps), rb, snap(rps))
        check_state(what, opt, ps, ropt, rps)
        assert ps[D]._version == vers[D] and torch.equal(ps[D].detach().cpu(), init[D]) and ps[D] not in opt.state
        if k == 1:
            assert ps[C]._version == vers[C] and torch.equal(ps[C].detach(), c_bits)
        assert bufA[0].item() == 0.0  # nothing was written in front of the misaligned parameter
    o = opt._offsets[next(i for i, p in enumerate(opt._params) if p is ps[D])]  # its slice of the flat state buffers
    assert not opt._exp_avg[o:o + shapes[D][0]].any() and not opt._exp_avg_sq[o:o + shapes[D][0]].any()


def test_versions_bumped_and_packer_sees_update():
    """the kernels write through raw pointers: every updated Parameter's _version must move, or MTLoRALinear would keep serving the
    factors a FactorPacker packed before the step."""
    from mtlora_amd.lora import FactorPacker, MTLoRALinear
    from mtlora_amd.optim import FusedAdamW
    init, grads = common_inputs()
    ps, opt = make_hip(init)
    for k in range(2):
        set_grads(ps, grads[1])
        vers = [p._version for p in ps]
        opt.clip_and_step(MAX_NORM)
        assert all(p._version > v for p, v in zip(ps, vers))

    def layer():
        torch.manual_seed(3)
        m = MTLoRALinear(96, 96, r=4, lora_shared_scale=2.0).to(dev()).train()
        m.linear.weight.requires_grad_(False)
        m.linear.bias.requires_grad_(False)
        with torch.no_grad():
            m.lora_shared_B.normal_(0.0, 0.5)
        return m

    lin = layer()
    x = torch.randn(64, 96, device=dev()).bfloat16()
    y0 = lin(x)[0]
    y0.float().pow(2).sum().backward()
    assert FactorPacker(lin).refresh() == 1
    y1 = lin(x)[0].detach().clone()
    assert lin._packed is not None and lin._packed_sig[1] == tuple(q._version for q in lin._factor_params())  # served from the pack
    FusedAdamW([lin.lora_shared_A, lin.lora_shared_B], lr=1e-2).step()
    y2 = lin(x)[0].detach().clone()  # no refresh() in between
    fresh = layer()
    with torch.no_grad():
        fresh.lora_shared_A.copy_(lin.lora_shared_A)
        fresh.lora_shared_B.copy_(lin.lora_shared_B)
    y3 = fresh(x)[0].detach()
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, y3)


def test_loss_scaler_skip_backoff_growth():
    """LossScaler(init_scale=1024, growth_interval=2), gradients pre-multiplied by the scale: a good step, a step with one inf (skipped
    bit-exactly, scale 512, tracker 0), two good steps (scale back to 1024; the bias corrections continue from the un-incremented
    step: the reference skipped too)."""
    from mtlora_amd.optim import LossScaler
    init, _ = common_inputs()
    _, grads = common_inputs(scales=(0.01, 0.01, 30.0, 0.01), seed=2)
    ps, opt = make_hip(init)
    rps, ropt = make_ref(init)
    scaler = LossScaler(init_scale=1024.0, growth_interval=2)
    expect = [(1024.0, 1), (512.0, 0), (512.0, 1), (1024.0, 0)]  # (scale, tracker) after each call
    for k, gs in enumerate(grads):
        scale = scaler.get_scale()
        set_grads(ps, gs, mult=scale)
        before, rb = snap(ps), snap(rps)
        what = f"loss scaler call {k + 1} (scale {scale:g})"
        if k == 1:
            ps[5].grad[1234] = float("inf")
            assert SHAPES[5] == (4097,)
            bits = [p.detach().clone() for p in ps]
            m_bits, v_bits, step = opt._exp_avg.clone(), opt._exp_avg_sq.clone(), opt.state[ps[0]]["step"].item()
            norm = opt.clip_and_step(MAX_NORM, scaler)
            assert not torch.isfinite(norm).item()
            assert all(torch.equal(p.detach(), b) for p, b in zip(ps, bits))
            assert torch.equal(opt._exp_avg, m_bits) and torch.equal(opt._exp_avg_sq, v_bits)
            assert opt.state[ps[0]]["step"].item() == step == 1
        else:
            norm = opt.clip_and_step(MAX_NORM, scaler)
            rnorm = ref_step(rps, ropt, gs)
            check_norm(what, norm, rnorm)
            check_delta(what, before, snap(ps), rb, snap(rps))
            check_state(what, opt, ps, ropt, rps)
        sd = scaler.state_dict()
        assert (sd["scale"], sd["_growth_tracker"]) == expect[k], (k, sd)
    assert opt.state[ps[0]]["step"].item() == 3
    assert set(scaler.state_dict()) == set(torch.amp.GradScaler("cuda").state_dict())
    loss = torch.ones((), device=dev(), requires_grad=True)
    assert scaler.scale(loss).item() == 1024.0


def test_state_dict_interchanges_with_torch_adamw():
    """a checkpoint written by either optimizer loads into the other: same keys, and both continue alike"""
    from mtlora_amd.optim import FusedAdamW
    init, _ = common_inputs()
    _, grads = common_inputs(scales=(0.01, 30.0, 0.01, 30.0), seed=4)
    ps, opt = make_hip(init)
    for k in range(2):
        set_grads(ps, grads[k])
        opt.clip_and_step(MAX_NORM)
    sd = opt.state_dict()

    def torch_twin(src):
        qs = [torch.nn.Parameter(p.detach().clone()) for p in src]
        return qs, torch.optim.AdamW(groups_of(qs), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=False)

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
        check_norm(what, norm, tnorm.double().cpu())
        check_delta(what, before, snap(hip_ps), tb, snap(tps))

    both_step(2, ps, opt, "FusedAdamW state into torch AdamW, step 3")
    assert opt.state[ps[0]]["step"].item() == 3 and topt.state[tps[0]]["step"].item() == 3  # (state_dict() handed out copies)
    tsd = topt.state_dict()
    assert set(sd) == set(tsd) == set(native)
    assert all(set(a) == set(b) for a, b in zip(sd["param_groups"], native["param_groups"]))
    assert set(sd["state"]) == set(tsd["state"]) and all(set(sd["state"][i]) == set(tsd["state"][i]) for i in sd["state"])
    # the other direction: torch's three steps into a new FusedAdamW over copies of torch's parameters
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in tps]
    opt2 = FusedAdamW(groups_of(ps2), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    opt2.load_state_dict(tsd)
    assert opt2.state[ps2[0]]["step"].item() == 3
    both_step(3, ps2, opt2, "torch AdamW state into FusedAdamW, step 4")
    # one counter for all parameters: unequal steps are refused, and nothing was touched
    tsd = topt.state_dict()
    tsd["state"][0]["step"] = tsd["state"][0]["step"] + 1
    m_bits = opt2._exp_avg.clone()
    with pytest.raises(ValueError, match="one step counter"):
        opt2.load_state_dict(tsd)
    assert torch.equal(opt2._exp_avg, m_bits) and opt2.state[ps2[0]]["step"].item() == 4


def _manual_forward_backward(model, crit, img, tg):
    """forward + backward exactly as mtl_harness.train_step issues them, without its optimizer part"""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    Fn.droppath_begin_step(img.device)
    H._factor_packer(model).refresh()
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _ = crit.combine(model(img, upsample=False, per_task_fn=lambda t, lo: crit.task_low(t, lo, tg[t])))
    finally:
        Fn.droppath_end_step()
    side = H._factor_side_stream(img.device)
    Fn.set_factor_stream(side)
    try:
        loss.backward()
    finally:
        Fn.set_factor_stream(None)
    if side is not None:
        torch.cuda.current_stream(img.device).wait_stream(side)
        Fn.factor_stream_joined()
    return loss.detach()


def test_train_step_hip_optimizer_and_accumulation():
    """train_step with build_optimizer(impl="hip") against the torch path on the same GPU gradients; gradient accumulation
    (update_grad=False keeps the gradients and updates nothing); fp16 autocast with the LossScaler."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW, LossScaler
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=13, device=dev())
    img2, tg2 = H.synthetic_batch(2, 224, tasks, seed=14, device=dev())

    def fresh(impl):
        torch.manual_seed(5)
        Fn._seed_counter = 0
        Fn.droppath_reset()
        model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, seed=3).to(dev()).train()
        return model, H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl=impl)

    def named(model):
        return {n: p.detach().double().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}

    def compare(what, before, hip_after, torch_after):
        names = list(before)
        check_delta(what, [before[n] for n in names], [hip_after[n] for n in names], [before[n] for n in names],
                    [torch_after[n] for n in names], names)

    # (a) one step
    out = {}
    for impl in ("torch", "hip"):
        model, crit, opt = fresh(impl)
        assert isinstance(opt, FusedAdamW) == (impl == "hip")
        before = named(model)
        loss, norm = H.train_step(model, crit, opt, img, tg)
        assert all(p.grad is None for p in model.parameters())
        out[impl] = (loss.clone(), norm.clone(), before, named(model))
    assert torch.equal(out["hip"][0], out["torch"][0])
    check_norm("train_step: norm against clip_grad_norm_ (fp32, GPU)", out["hip"][1], out["torch"][1].double().cpu())
    assert all(torch.equal(out["hip"][2][n], out["torch"][2][n]) for n in out["hip"][2])
    compare("train_step: one step against torch fused AdamW", out["hip"][2], out["hip"][3], out["torch"][3])
    bf16_loss = out["hip"][0].item()

    # (b) two micro-batches, one update
    model, crit, opt = fresh("torch")
    before = named(model)
    _manual_forward_backward(model, crit, img, tg)
    _manual_forward_backward(model, crit, img2, tg2)
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    tnorm = torch.nn.utils.clip_grad_norm_(params, 5.0, foreach=True)
    opt.step()
    torch_after = named(model)
    model, crit, opt = fresh("hip")
    l1, n1 = H.train_step(model, crit, opt, img, tg, update_grad=False)
    assert n1 is None and torch.isfinite(l1).item()
    mid = named(model)
    assert all(torch.equal(mid[n], before[n]) for n in before)
    assert sum(p.grad is not None for p in model.parameters()) == len(params)
    l2, n2 = H.train_step(model, crit, opt, img2, tg2)
    check_norm("accumulation: norm of the summed gradients", n2, tnorm.double().cpu())
    compare("accumulation: update after two micro-batches", before, named(model), torch_after)

    # (c) the reference's default AMP mode: fp16 autocast + loss scaler
    model, crit, opt = fresh("hip")
    scaler = LossScaler(init_scale=1024.0)
    losses = [H.train_step(model, crit, opt, img, tg, amp_dtype=torch.float16, loss_scaler=scaler)[0].item() for _ in range(2)]
    assert all(np.isfinite(v) for v in losses), losses
    assert scaler.get_scale() >= 1024.0  # no step was skipped
    fig("fp16 + LossScaler: first loss against bf16, relative", abs(losses[0] - bf16_loss) / abs(bf16_loss))
    assert abs(losses[0] - bf16_loss) <= 2e-2 * abs(bf16_loss), (losses[0], bf16_loss)
