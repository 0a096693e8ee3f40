"""Trainable LoRA scales (TRAINABLE_SCALE_SHARED / TRAINABLE_SCALE_PER_TASK) on the device: the packing launch reads the 1-element
Parameters, the scale gradients come from mtlora_linear_scale_grad, and nothing on the path reads a scale on the host -- so the layer
runs without a synchronisation, inside a captured graph that follows the Parameters, and through the FactorPacker's one launch.

Shapes: M = 98 (two 7 x 7 windows; no multiple of 32 or 64), (K, N) in {(96, 288), (384, 96)}, r_s in {8, 64}, r_t = 4, T in {0, 3} with
and without x_tasks, 'matrix' and 'matrixv2', fp32 / bf16 / fp16, eval and train (lora_dropout 0.05 at a fixed seed)."""
import ctypes
import functools

import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

M = 98
GEOMS = [(96, 288), (384, 96)]
RANKS = [8, 64]
CFGS = [(0, False, "matrix"), (3, False, "matrix"), (3, True, "matrix"), (3, False, "matrixv2"), (3, True, "matrixv2")]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
P_DROP = 0.05
SCALES = (2.7, 1.3, 0.9, 3.1)  # shared, then the tasks: distinct, none a power of two
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2, torch.float16: 1e-2}  # the kernel tolerances, max-norm relative


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def make_layer(K, N, rs, T, mode, trainable, dtype=torch.float32, seed=0, p=P_DROP):
    from mtlora_amd.lora import MTLoRALinear
    tasks = [f"t{i}" for i in range(T)] or None
    torch.manual_seed(1000 + seed)
    r = {"shared": rs, **{t: 4 for t in (tasks or [])}}
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()  # the constant twin gets exactly the float the Parameter holds
    m = MTLoRALinear(K, N, r=r, lora_shared_scale=f32(SCALES[0]),
                     lora_task_scale={t: f32(SCALES[1 + i]) for i, t in enumerate(tasks)} if tasks else 1.0, lora_dropout=p, tasks=tasks,
                     trainable_scale_shared=trainable, trainable_scale_per_task=trainable, shared_mode=mode).to(dev())
    with torch.no_grad():
        for n, q in m.named_parameters():
            if "scale" in n:
                continue
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n else 0.02))
            if dtype != torch.float32:
                q.copy_(q.to(dtype).float())  # parameters exactly representable: only the accumulation order differs
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    return m


def inputs(K, N, T, use_xt, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(77 + seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev()).to(dtype)
    x = mk(M, K)
    xt = [mk(M, K) for _ in range(T)] if use_xt else None
    gy = [mk(M, N) for _ in range(1 + T)]
    return x, xt, gy


def run_layer(m, x, xt, gy, seed_counter=None):
    """forward + backward of sum_o <y_o, gy_o>, or with gy None of sum_o |y_o|^2 / 2; returns every output and gradient by name"""
    from mtlora_amd import functional as Fn
    tasks = list(m.tasks) if m.tasks else []
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    xtd = {t: v.detach().clone().requires_grad_(True) for t, v in zip(tasks, xt)} if xt is not None else None
    if seed_counter is not None:
        Fn._seed_counter = seed_counter
    y, yt = m(x, xtd)
    if gy is None:
        loss = 0.5 * (y.float() ** 2).sum() + sum(0.5 * (yt[t].float() ** 2).sum() for t in tasks)
    else:
        loss = (y.float() * gy[0].float()).sum()
        for i, t in enumerate(tasks):
            loss = loss + (yt[t].float() * gy[1 + i].float()).sum()
    loss.backward()
    out = {"y": y.detach(), "dx": x.grad}
    for t in tasks:
        out["y." + t] = yt[t].detach()
        if xtd is not None:
            out["dx." + t] = xtd[t].grad
    for n, q in m.named_parameters():
        if q.requires_grad:
            out["grad." + n] = q.grad
    return out


@functools.lru_cache(maxsize=None)
def case(K, N, rs, T, use_xt, mode, dtype, train):
    """one configuration, run once for every test that looks at it: the layer with device scales, its constant-scale twin, and the
    fp64 oracle with autograd on the scales.

    The loss is sum_o |y_o|^2 / 2, not a random projection sum_o <y_o, g_o>.  A scale's gradient is ONE number, <dB, B> / s = <dY, U>
    (U the unscaled update).  With g independent of the layer that number is a sum of N r zero-mean terms: its expectation is 0, its
    condition number sum|t| / |sum t| grows like sqrt(N r) (50 .. 200 here), and the relative error of the single number is then that
    many times the 2^-9 roundings of the 16-bit intermediates P, Q, G whatever the kernel does -- measured on the MI355X with the
    random projection: fp32 <= 1.1e-6, bf16 up to 4.6e-2 (96x288 r8 T3 x_tasks matrixv2 train: -1.7687 against -1.8535), from the
    same dB bits the ATen formula of the earlier code reads.  With dY = Y the number contains s |U|^2 > 0, which dominates the
    cross terms (|s U| ~ |X W^T| for these fills), so it is well conditioned and the kernel tolerance on it means what it means
    for a tensor: rounding of the path, not cancellation in the test's own data."""
    from mtlora_amd import functional as Fn
    a, b = make_layer(K, N, rs, T, mode, True, dtype), make_layer(K, N, rs, T, mode, False, dtype)
    with torch.no_grad():
        for (n, q) in b.named_parameters():
            q.copy_(dict(a.named_parameters())[n])
    a.train(train), b.train(train)
    x, xt, gy = inputs(K, N, T, use_xt, dtype)
    got = run_layer(a, x, xt, None, seed_counter=41)
    twin = run_layer(b, x, xt, None, seed_counter=41)
    torch.cuda.synchronize()
    # the oracle: every parameter (the scales included) in fp64 with autograd, the kernel's dropout mask restated
    tasks = list(a.tasks) if a.tasks else None
    P = {n: q.detach().double().cpu().requires_grad_(q.requires_grad) for n, q in a.named_parameters()}
    keep = None
    if train:
        Fn._seed_counter = 41
        keep = O.dropout_keep_mask(Fn.next_seed(), 0, M, K, P_DROP)
    xs = x.double().cpu()
    xts = {t: v.double().cpu() for t, v in zip(tasks, xt)} if (tasks and xt is not None) else None
    yo, yto = O.mtlora_linear(xs, P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], P["lora_shared_scale"],
                              tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks} if tasks else None,
                              B_t={t: P["lora_tasks_B." + t] for t in tasks} if tasks else None,
                              scale_t={t: P["lora_task_scale." + t] for t in tasks} if tasks else None, x_tasks=xts, shared_mode=mode,
                              keep_mask=keep, p=P_DROP if train else 0.0)
    lo = 0.5 * (yo ** 2).sum() + sum(0.5 * (yto[t] ** 2).sum() for t in (tasks or []))
    lo.backward()
    ref = {"grad." + n: q.grad for n, q in P.items() if q.requires_grad}
    return got, twin, ref


def dict_param(c, grad_name):
    """the value of the parameter a gradient name of ``case`` belongs to (the layers are rebuilt from the same seed)"""
    K, N, rs, T, _, mode, dtype, _ = c
    return dict(make_layer(K, N, rs, T, mode, True, dtype).named_parameters())[grad_name[len("grad."):]].detach().double().cpu()


ALL = [(K, N, rs, T, xt, mode, dt, tr) for (K, N) in GEOMS for rs in RANKS for (T, xt, mode) in CFGS for dt in DTYPES for tr in (False, True)]
_id = lambda c: f"{c[0]}x{c[1]}-r{c[2]}-T{c[3]}{'xt' if c[4] else ''}-{c[5]}-{str(c[6]).split('.')[-1]}-{'train' if c[7] else 'eval'}"


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_device_scales_are_bit_identical_to_constant_scales(c):
    """1. a layer whose scale Parameters hold s against its twin built with the constants float(s): y, every y_t, dx, every dx_t and
    every dA / dB are torch.equal (the packing kernel forms the same fp32 product the host forms by value)"""
    got, twin, _ = case(*c)
    for n, v in twin.items():
        assert torch.equal(got[n], v), n
    assert {n for n in got if n not in twin} == {n for n in got if "scale" in n}


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_scale_gradients_match_the_fp64_oracle(c):
    """2. d(loss)/d(scale) of every segment against oracle/mtlora_oracle.py with autograd on the scales, at the kernel tolerances"""
    got, _, ref = case(*c)
    names = [n for n in got if "scale" in n]
    assert len(names) == 1 + c[3]
    for n in names:
        assert got[n] is not None and got[n].shape == (1,) and torch.isfinite(got[n]).all(), n
        e = rel_err(got[n], ref[n])
        Bn = n.replace("lora_shared_scale", "lora_shared_B").replace("lora_task_scale.", "lora_tasks_B.")
        t = got[Bn].double().cpu() * dict_param(c, Bn)
        print(n, got[n].item(), ref[n].item(), e, "condition", (t.abs().sum() / t.sum().abs()).item())
        assert e <= TOL[c[6]], f"{n}: rel err {e:.3e} > {TOL[c[6]]:.0e}"


@pytest.mark.parametrize("geom", [(96, 288, 8, 3), (384, 96, 64, 3), (96, 288, 64, 0)])
def test_scale_grad_kernel_against_the_portable_definition(geom):
    """2b. mtlora_linear_scale_grad against functional.scale_grad_torch on the same fp32 dB, B: only the summation order differs
    (1e-6 relative); a zero scale gives 0, a segment with a null dB or a null scale keeps its word, and two runs give the same bits"""
    from mtlora_amd import _lib as L
    from mtlora_amd import functional as Fn
    K, N, rs, T = geom
    g = torch.Generator(device="cpu").manual_seed(5)
    ranks = [rs] + [4] * T
    B = [torch.randn(N, r, generator=g).to(dev()) for r in ranks]
    # (dB correlated with B, as a gradient of s B (..) is: <dB, B> is then no zero-mean sum whose relative error measures its own
    # cancellation -- with independent draws the fp32 partial sums were 3.3e-5 off a total 200 times smaller than sum |dB B|)
    dB = [(0.5 * b.cpu() + 0.1 * torch.randn(N, r, generator=g)).to(dev()) for b, r in zip(B, ranks)]
    sc = [torch.tensor([v], device=dev()) for v in SCALES[:1 + T]]
    meta = Fn.LinearMeta(K=K, N=N, r_s=rs, r_t=(4,) * T, scale_s=sc[0], scale_t=tuple(sc[1:]), mode=0, has_x_tasks=False, dropout_p=0.0,
                         seed=0, dtype=torch.float32)
    d = meta.desc(1)
    scratch = torch.empty(L.lib().mtlora_linear_scale_grad_scratch_bytes(), dtype=torch.uint8, device=dev())

    def run(dBs, scs):
        out = torch.full((1 + T,), 123.0, device=dev())
        st = L.lib().mtlora_linear_scale_grad(ctypes.byref(d), L.ptr_array9(dBs), L.ptr_array9(B), L.ptr_array9(scs), 1 + T, L.ptr(out),
                                              L.ptr(scratch), scratch.numel(), L.stream_ptr())
        assert st == 0, st
        return out

    out = run(dB, sc)
    for o in range(1 + T):
        want = Fn.scale_grad_torch(dB[o], B[o], sc[o])
        e = rel_err(out[o:o + 1], want)
        print(o, out[o].item(), want.item(), e)
        assert e <= 1e-6, (o, e)
    assert torch.equal(run(dB, sc), out)
    zero = [torch.zeros(1, device=dev())] + sc[1:]
    assert run(dB, zero)[0].item() == 0.0 and Fn.scale_grad_torch(dB[0], B[0], zero[0]).item() == 0.0
    if T:
        part = run([dB[0], None] + dB[2:], sc[:2] + [None] + sc[3:])
        assert part[1].item() == 123.0 and part[2].item() == 123.0 and part[0].item() == out[0].item() and part[3].item() == out[3].item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_frozen_B_still_gives_the_scale_its_gradient(dtype):
    """2c. B.requires_grad = False (shared and one task): the scales' gradients are there and match the oracle, B.grad is None"""
    K, N, rs, T = 96, 288, 8, 3
    got, _, ref = case(K, N, rs, T, True, "matrix", dtype, False)
    m = make_layer(K, N, rs, T, "matrix", True, dtype).eval()
    m.lora_shared_B.requires_grad_(False)
    m.lora_tasks_B["t1"].requires_grad_(False)
    x, xt, gy = inputs(K, N, T, True, dtype)
    out = run_layer(m, x, xt, None)
    assert m.lora_shared_B.grad is None and m.lora_tasks_B["t1"].grad is None
    assert "grad.lora_shared_B" not in out and "grad.lora_tasks_B.t1" not in out
    for n in [k for k in got if "scale" in k]:
        assert out[n] is not None, n
        assert torch.equal(out[n], got[n]), n  # the same launches as with a trained B
        assert rel_err(out[n], ref[n]) <= TOL[dtype], n
    for n in ("grad.lora_shared_A", "grad.lora_tasks_B.t0", "grad.lora_tasks_A.t1", "dx"):
        assert torch.equal(out[n], got[n]), n


def test_forward_and_backward_make_no_host_sync():
    """3. forward + backward of a trainable-scale layer under torch.cuda.set_sync_debug_mode("error")"""
    K, N, rs, T = 96, 288, 8, 3
    m = make_layer(K, N, rs, T, "matrix", True, torch.bfloat16).train()
    x, xt, gy = inputs(K, N, T, True, torch.bfloat16)
    want = run_layer(m, x, xt, gy, seed_counter=7)  # (warm: allocator, library load)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run_layer(m, x, xt, gy, seed_counter=7)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    for n, v in want.items():
        assert torch.equal(got[n], v), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_layer_follows_the_scale_parameters(dtype):
    """4. forward + backward of one layer captured with torch.cuda.graph; the scales are changed by a device-side in-place op and the
    graph is replayed: outputs and gradients equal an eager call at the new values, twice"""
    K, N, rs, T = 384, 96, 64, 3
    m = make_layer(K, N, rs, T, "matrixv2", True, dtype).eval()
    x, xt, gy = inputs(K, N, T, True, dtype)
    tasks = list(m.tasks)
    params = [q for q in m.parameters() if q.requires_grad]
    xs = x.clone().requires_grad_(True)
    xts = {t: v.clone().requires_grad_(True) for t, v in zip(tasks, xt)}

    def step():
        y, yt = m(xs, xts)
        loss = (y.float() * gy[0].float()).sum()
        for i, t in enumerate(tasks):
            loss = loss + (yt[t].float() * gy[1 + i].float()).sum()
        grads = torch.autograd.grad(loss, [xs, *xts.values(), *params])
        return [y, *yt.values(), *grads]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    scales = [m.lora_shared_scale] + [m.lora_task_scale[t] for t in tasks]
    for k, f in enumerate((1.37, 0.61)):
        with torch.no_grad():
            for i, s in enumerate(scales):
                s.mul_(f + 0.05 * i)  # (a device-side in-place op: no host value enters)
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step()
        torch.cuda.synchronize()
        assert len(got) == len(want) == 1 + T + 1 + T + len(params)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (k, i)


def test_factor_packer_packs_and_tracks_trainable_scale_layers():
    """5. FactorPacker.refresh() counts the trainable-scale layers; after an in-place change of a scale plus refresh() the forward
    equals the same layer run without a packer; without the refresh() the layer notices the stale version and packs inside the call"""
    import torch.nn as nn
    from mtlora_amd.lora import FactorPacker
    K, N = 96, 288
    x, xt, gy = inputs(K, N, 3, True, torch.bfloat16)
    layers = [make_layer(K, N, 8, 3, "matrix", True, torch.bfloat16, seed=1).eval(),
              make_layer(K, N, 64, 0, "matrix", True, torch.bfloat16, seed=2).eval(),
              make_layer(K, N, 8, 3, "matrix", False, torch.bfloat16, seed=3).eval()]
    model = nn.ModuleList(layers)

    def fwd():
        with torch.no_grad():
            outs = []
            for m in layers:
                y, yt = m(x, {t: v for t, v in zip(m.tasks, xt)} if m.tasks else None)
                outs += [y] + (list(yt.values()) if yt else [])
            return outs

    plain = fwd()  # (no packer yet: every layer packs inside the call; also records the call signatures)
    pk = FactorPacker(model)
    assert pk.refresh() == 3
    assert all(m._packed is not None and m._packed_sig == (m._call_sig, m._versions()) for m in layers)
    for a, b in zip(fwd(), plain):
        assert torch.equal(a, b)
    with torch.no_grad():
        layers[0].lora_shared_scale.mul_(1.7)
        layers[0].lora_task_scale["t2"].add_(0.3)
        layers[1].lora_shared_scale.mul_(0.4)
    # stale: the layers must not use the packer's buffers
    assert all(m._packed_sig != (m._call_sig, m._versions()) for m in layers[:2])
    stale = fwd()
    assert not torch.equal(stale[0], plain[0]) and not torch.equal(stale[4], plain[4]) and torch.equal(stale[5], plain[5])
    for m in layers:
        m._packed_sig = None  # (what invalidate_weight_cache does: no buffer of the packer counts as current)
    want = fwd()  # (the same layers without a packer)
    for a, b in zip(stale, want):
        assert torch.equal(a, b)
    assert pk.refresh() == 3
    assert all(m._packed is not None and m._packed_sig == (m._call_sig, m._versions()) for m in layers)
    for a, b in zip(fwd(), want):
        assert torch.equal(a, b)


def test_whole_model_graphed_train_step_with_trainable_scales():
    """6. the model of test_gpu_models.test_graphed_train_step_replays_the_eager_step with both TRAINABLE_SCALE_* flags and
    FusedAdamW(capturable=True): three GraphedTrainStep replays against three eager steps of the same step object from the same
    state, by that test's criterion (losses within 2e-3 relative, cosine of the accumulated updates >= 0.98); every scale Parameter
    has moved and has a finite gradient.  "Every": every scale whose segment takes part in the loss.  The shared output of the last
    block's fc2 feeds nothing when there are tasks (the heads read the task streams), in the reference as here, so that one
    segment's B and scale get no gradient and stand still; the test therefore asks of each scale exactly what holds for the B of
    its segment (moved iff B moved, a gradient iff B has one) and that at most that one segment stands still."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=17, device=dev())
    out = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=4,
                              TRAINABLE_SCALE_SHARED=True, TRAINABLE_SCALE_PER_TASK=True).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        assert isinstance(opt, FusedAdamW)
        scales = {n: p for n, p in model.named_parameters() if "lora_shared_scale" in n or "lora_task_scale" in n}
        assert len(scales) > 8 and all(p.requires_grad and p.numel() == 1 for p in scales.values())
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2)
            assert gs.graphed, gs.why
            if not use_graph:
                gs.graphed = False  # the same object's eager path (same seed-offset walk)
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses = [gs().clone() for _ in range(3)]
            torch.cuda.synchronize()
            out.append((losses, {n: (p.detach() - start[n]).double() for n, p in model.named_parameters() if n in start}))
            B_of = lambda n: n.replace("lora_shared_scale", "lora_shared_B").replace("lora_task_scale.", "lora_tasks_B.")
            params = dict(model.named_parameters())
            still = [n for n, p in scales.items() if torch.equal(p.detach(), start[n])]
            assert still == [n for n in scales if torch.equal(params[B_of(n)].detach(), start[B_of(n)])], still
            assert len(still) <= 1 and all(n.endswith("mlp.fc2.lora_shared_scale") for n in still), still
            if not use_graph:  # the gradients themselves: one more forward + backward without an update
                H.train_step(model, crit, opt, img, tg, update_grad=False)
                torch.cuda.synchronize()
                for n, p in scales.items():
                    assert (p.grad is None) == (params[B_of(n)].grad is None) == (n in still), n
                    assert p.grad is None or torch.isfinite(p.grad).all(), n
                opt.zero_grad(set_to_none=True)
        finally:
            Fn.set_seed_offset(None)
    for a, b in zip(out[0][0], out[1][0]):
        print("loss", a.item(), b.item())
        assert abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    num = sum((out[0][1][n] * out[1][1][n]).sum().item() for n in out[0][1])
    den = (sum((out[0][1][n] ** 2).sum().item() for n in out[0][1]) * sum((out[1][1][n] ** 2).sum().item() for n in out[1][1])) ** 0.5
    print("cosine", num / den)
    assert num / den >= 0.98, num / den
