"""Full fine-tuning on the HIP path (MODEL.MTLORA.FREEZE_PRETRAINED False): ``mtlora_linear_weight_grad`` and
``mtlora_linear_weight_cast`` (csrc/weight_grad.hip) against fp64 and against ``W.to(dtype)``, the per-layer autograd path, the
fc1 -> GELU -> fc2 pairing, the per-call refresh of a trainable W, the whole backbone and a captured train step.

Bounds, none of them new: the kernel against the fp64 product of the SAME rounded inputs at the kernel-parity bound of
test_gpu_linear_bias.py (max-norm relative 1e-3; accumulation is fp32 for every dtype, so one bound serves all three); layer-level
gradients at the file-wide bounds of test_gpu_kernels.py (1e-3 fp32, 1e-2 bf16); the backbone at the bounds of
test_gpu_models.test_bias_all_trains_frozen_linears_biases (2e-3 fp32, 1e-2 under bf16 autocast); the captured step by the criterion
of test_gpu_optim_capturable.test_whole_step_graphed_with_scaler."""
import ctypes
import math

import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}
ERR_SHAPE, ERR_ALIGN, ERR_WORKSPACE = -2, -3, -5


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def weight_grad(x, srcs, M, N, K, dtype, scratch_short=0):
    """(status, dW, size query) of one mtlora_linear_weight_grad call; srcs = [dy_s, dy_t[0], ...], None for an output without a
    gradient.  dW is poisoned with NaN: whatever comes back finite was written by the call."""
    from mtlora_amd import _lib as L
    lib = L.lib()
    d = L.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T = M, K, N, L._DT[dtype], len(srcs) - 1
    sb = lib.mtlora_linear_weight_grad_scratch_bytes(ctypes.byref(d))
    dW = torch.full((N, K), float("nan"), dtype=torch.float32, device=dev())
    scratch = torch.empty(max(sb, 16), dtype=torch.uint8, device=dev())  # (sb < 0: a refused shape; the call must refuse it as well)
    st = lib.mtlora_linear_weight_grad(ctypes.byref(d), L.ptr(x), L.ptr(srcs[0]), L.ptr_array(srcs[1:]), L.ptr(dW), L.ptr(scratch),
                                       sb - scratch_short, L.stream_ptr())
    return st, dW, sb


# (M, N, K, present sources out of [dy_s, dy_t...]): one case per branch of the walk over 128 x 128 tiles and 64- (fp32: 32-) row chunks
CASES = {
    "one_row_one_vector": (1, 8, 8, [True]),
    "ragged_tile_and_chunk": (197, 104, 72, [True]),                        # one partial tile, M no multiple of a chunk
    "tiles_5x3_task_source_missing": (2 * 49, 520, 264, [True, True, False]),  # a ragged last tile both ways, quadrants switched off
    "shared_source_missing": (64, 384, 96, [False, True]),
    "split_m_ragged_last_split": (8200, 96, 32, [True, True]),              # 15 splits of 576 rows, the last one 136 rows; k_tn_reduce
    "no_split_stage3_aspect": (64, 768, 768, [True]),                       # 36 tiles, one split: the direct store
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_vs_fp64_product(case, dtype):
    M, N, K, present = CASES[case]
    g = torch.Generator().manual_seed(M * 131 + N + K)
    x = torch.randn(M, K, generator=g).to(dtype).to(dev())
    srcs = [torch.randn(M, N, generator=g).to(dtype).to(dev()) if on else None for on in present]
    ref = sum(s.double() for s in srcs if s is not None).t() @ x.double()
    st, dW, sb = weight_grad(x, srcs, M, N, K, dtype)
    assert st == 0
    if case == "split_m_ragged_last_split":
        assert sb >= 15 * 128 * 128 * 4  # (the split branch: partial tiles)
    elif M <= 512:
        assert sb < 128 * 128 * 4        # (no split: no partial tiles)
    err = rel_err(dW, ref)
    print(f"weight_grad {case} {dtype}: rel err {err:.3e}")
    assert err <= 1e-3, err
    st2, dW2, _ = weight_grad(x, srcs, M, N, K, dtype)
    assert st2 == 0 and torch.equal(dW.view(torch.int32), dW2.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_kernel_writes_zeros_without_sources_or_rows(dtype):
    x = torch.ones(64, 96, device=dev()).to(dtype)
    st, dW, _ = weight_grad(x, [None, None, None], 64, 384, 96, dtype)
    assert st == 0 and torch.equal(dW, torch.zeros_like(dW))  # (dW was poisoned with NaN: the kernel wrote every element)
    rows = torch.ones(8, 384, device=dev()).to(dtype)         # valid addresses; M = 0 reads none of them
    st, dW, _ = weight_grad(x, [rows, rows], 0, 384, 96, dtype)
    assert st == 0 and torch.equal(dW, torch.zeros_like(dW))


def test_kernel_argument_errors():
    bf = torch.bfloat16
    x = torch.ones(16, 24, device=dev(), dtype=bf)
    st, _, sb = weight_grad(x, [x[:, :12].contiguous()], 16, 12, 24, bf)  # N = 12: 1.5 vectors per row
    assert st == ERR_SHAPE and sb == -1
    flat = torch.ones(16 * 24 + 8, device=dev(), dtype=bf)
    assert weight_grad(x, [flat[1:]], 16, 24, 24, bf)[0] == ERR_ALIGN      # 2 bytes off the 16-byte grid
    assert weight_grad(x, [x], 16, 24, 24, bf, scratch_short=1)[0] == ERR_WORKSPACE
    st, dW, _ = weight_grad(x, [x], 16, 24, 24, bf)
    assert st == 0 and torch.equal(dW, torch.full_like(dW, 16.0))


# ----------------------------------------------------------------------------------------------
# the cast entry
# ----------------------------------------------------------------------------------------------
def _tie_master(N, K):
    """randn with values that sit exactly between two neighbours of bf16 (0x3F808000 rounds down to even, 0x3F818000 up to even) and of
    fp16 (0x3F801000 down, 0x3F803000 up), both signs, mixed in"""
    g = torch.Generator().manual_seed(N * 7 + K)
    w = torch.randn(N, K, generator=g)
    bits = torch.tensor([0x3F808000, 0x3F818000, 0x3F801000, 0x3F803000], dtype=torch.int64)
    ties = torch.cat([bits, bits | 0x80000000]).to(torch.int32).view(torch.float32)  # (the int64 -> int32 cast wraps the sign bit in)
    flat = w.view(-1)
    idx = torch.arange(0, flat.numel(), 5)
    flat[idx] = ties[torch.arange(idx.numel()) % ties.numel()]
    return w


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(8, 8), (96, 288), (104, 72)], ids=["8x8", "96x288", "104x72_off_tile"])
def test_weight_cast_is_bit_equal_to_torch(shape, dtype):
    from mtlora_amd import functional as Fn
    N, K = shape
    W = _tie_master(N, K).to(dev())
    wc = torch.full((N, K), float("nan"), dtype=dtype, device=dev())
    wt = torch.full((K, N), float("nan"), dtype=dtype, device=dev())
    Fn.weight_cast(W, wc, wt)
    view = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(wc.view(view), W.to(dtype).view(view))
    assert torch.equal(wt.view(view), W.t().to(dtype).contiguous().view(view))
    if dtype == torch.bfloat16:  # the ties went to even
        assert wc.view(-1)[0].item() == 1.0 and wc.view(-1)[5].view(torch.int16).item() == 0x3F82


# ----------------------------------------------------------------------------------------------
# the per-layer autograd path
# ----------------------------------------------------------------------------------------------
TASKS = ["a", "b"]


def _layer(shared_mode="matrix"):
    """the layer of test_gpu_linear_bias._layer(): 96 -> 288, r 8 / 4 / 4, two tasks"""
    from mtlora_amd import lora
    torch.manual_seed(11)
    m = lora.MTLoRALinear(96, 288, r={"shared": 8, "a": 4, "b": 4}, lora_shared_scale=2.0, lora_task_scale={"a": 1.5, "b": 0.5},
                          tasks=TASKS, shared_mode=shared_mode).to(dev())
    with torch.no_grad():
        for n, q in m.named_parameters():
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n else 0.02))
    return m.train()


def _run_layer(m, xs, gys, use_xt, amp):
    m.zero_grad(set_to_none=True)
    ins = [x.clone().requires_grad_(True) for x in xs[:1 + (len(TASKS) if use_xt else 0)]]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        y, yt = m(ins[0], {t: ins[1 + i] for i, t in enumerate(TASKS)} if use_xt else None)
    outs = [y] + [yt[t] for t in TASKS]
    torch.autograd.backward(outs, [g.to(o.dtype) for g, o in zip(gys, outs)])
    grads = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
    grads.update({f"x{i}": x.grad.clone() for i, x in enumerate(ins)})
    return grads


@pytest.fixture
def spy(monkeypatch):
    """counts the calls of mtlora_linear_weight_grad (without it the layer tests would pass on an ATen product)"""
    from mtlora_amd import _lib as L
    lib = L.lib()
    real, calls = lib.mtlora_linear_weight_grad, []

    def counted(*a):
        calls.append(1)
        return real(*a)

    monkeypatch.setattr(lib, "mtlora_linear_weight_grad", counted)
    return calls


@pytest.mark.parametrize("train_bias", [True, False], ids=["bias_trains", "bias_frozen"])
@pytest.mark.parametrize("mode", ["matrix", "matrixv2"])
@pytest.mark.parametrize("use_xt", [False, True], ids=["shared_input", "x_tasks"])
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16_autocast"])
def test_linear_layer_weight_gradient_vs_oracle(spy, amp, use_xt, mode, train_bias):
    """MTLoRALinear with a trainable W, M = 2 * 49: every gradient against the fp64 oracle at the layer bound, and every gradient other
    than dW and db bit-equal to the same call with W frozen (the refreshed copies are the frozen ones' bits, the new launch disturbs
    nothing)"""
    m = _layer(mode)
    M, dtype = 2 * 49, torch.bfloat16 if amp else torch.float32
    g = torch.Generator().manual_seed(3)
    xs = [(0.5 * torch.randn(M, 96, generator=g)).to(dev()) for _ in range(1 + len(TASKS))]
    gys = [torch.randn(M, 288, generator=g).to(dtype).float().to(dev()) for _ in range(1 + len(TASKS))]
    m.linear.bias.requires_grad_(train_bias)
    m.linear.weight.requires_grad_(True)
    got = _run_layer(m, xs, gys, use_xt, amp)
    assert len(spy) == 1
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    frozen = _run_layer(m, xs, gys, use_xt, amp)
    assert len(spy) == 1
    dense = {"linear.weight"} | ({"linear.bias"} if train_bias else set())
    assert set(got) - dense == set(frozen) and dense <= set(got)
    assert got["linear.weight"].dtype == torch.float32 and got["linear.weight"].shape == (288, 96)
    for n in frozen:
        assert torch.equal(got[n], frozen[n]), n
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    xo = [x.double().cpu().requires_grad_(True) for x in xs]
    yo, yto = O.mtlora_linear(xo[0], P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                              tasks=TASKS, A_t={t: P["lora_tasks_A." + t] for t in TASKS}, B_t={t: P["lora_tasks_B." + t] for t in TASKS},
                              scale_t=m.lora_task_scale, x_tasks={t: xo[1 + i] for i, t in enumerate(TASKS)} if use_xt else None,
                              shared_mode=mode)
    torch.autograd.backward([yo] + [yto[t] for t in TASKS], [g.double().cpu() for g in gys])
    ref = {k: v.grad for k, v in P.items()}
    ref.update({f"x{i}": x.grad for i, x in enumerate(xo)})
    for n in sorted(got):
        err = rel_err(got[n], ref[n])
        print(f"layer {n}.grad amp={amp} x_tasks={use_xt} {mode}: rel err {err:.3e}")
        assert err <= TOL[dtype], (n, err)


def test_mlp_pair_weight_gradients_vs_fp64(spy):
    """fc1 -> GELU -> fc2 through Mlp without tasks (C = 96, hidden 384, M = 98, bf16 autocast), both weights trainable: fc2's dW takes
    x2 = gelu(h), the operand its node saved, and fc1's the gradient that went through the fused gelu'"""
    from mtlora_amd.swin_transformer_mtlora import Mlp
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    torch.manual_seed(12)
    mlp = Mlp(96, 384, mtlora=mt, layer_idx=0).to(dev())
    with torch.no_grad():
        for n, q in mlp.named_parameters():
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n else 0.04))
    mlp.train()
    assert all(fc.linear.weight.requires_grad and fc.linear.bias.requires_grad for fc in (mlp.fc1, mlp.fc2))
    M = 2 * 49
    g = torch.Generator().manual_seed(4)
    x = torch.randn(M, 96, generator=g).to(dev()).requires_grad_(True)
    gy = torch.randn(M, 96, generator=g).to(torch.bfloat16).float().to(dev())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = mlp(x)[0]
    y.backward(gy.to(y.dtype))
    assert len(spy) == 2
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in mlp.named_parameters()}
    x64 = x.detach().double().cpu()
    h, _ = O.mtlora_linear(x64, P["fc1.linear.weight"], P["fc1.linear.bias"], P["fc1.lora_shared_A"], P["fc1.lora_shared_B"],
                           mlp.fc1.lora_shared_scale)
    yo, _ = O.mtlora_linear(torch.nn.functional.gelu(h), P["fc2.linear.weight"], P["fc2.linear.bias"], P["fc2.lora_shared_A"],
                            P["fc2.lora_shared_B"], mlp.fc2.lora_shared_scale)
    yo.backward(gy.double().cpu())
    for n in ("fc1.linear.weight", "fc2.linear.weight", "fc1.linear.bias", "fc2.linear.bias"):
        got = dict(mlp.named_parameters())[n].grad
        assert got is not None and got.dtype == torch.float32, n
        err = rel_err(got, P[n].grad)
        print(f"Mlp {n}.grad: rel err {err:.3e}")
        assert err <= TOL[torch.bfloat16], (n, err)


# ----------------------------------------------------------------------------------------------
# the per-call refresh of a trainable W
# ----------------------------------------------------------------------------------------------
def test_trainable_weight_copies_follow_a_raw_pointer_update():
    """two calls of a trainable layer with a FusedAdamW step (raw-pointer writes, whatever ``_version`` says) in between: the second forward
    sees the new weights through the SAME Wc / Wt buffers"""
    from mtlora_amd.optim import FusedAdamW
    m = _layer()
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=5e-2, weight_decay=0.0)
    x = torch.randn(98, 96, device=dev())
    key = (torch.bfloat16, m.linear.weight.device)
    seen = []
    for step in range(2):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y, yt = m(x)
        c = m._wcache[key]
        seen.append((c[1], c[2], c[1].data_ptr(), c[2].data_ptr(), c[1].clone(), y.detach().clone()))
        W = m.linear.weight.detach()
        assert torch.equal(c[1], W.to(torch.bfloat16)) and torch.equal(c[2], W.t().to(torch.bfloat16).contiguous())
        if step == 0:
            (y.float().square().mean() + sum(v.float().square().mean() for v in yt.values())).backward()
            w0 = W.clone()
            opt.step()
            assert not torch.equal(m.linear.weight.detach(), w0)
    (a, b) = seen
    assert a[0] is b[0] and a[1] is b[1] and a[2:4] == b[2:4]
    assert not torch.equal(a[4], b[0]) and not torch.equal(a[5], b[5])


def test_trainable_layer_used_twice_in_one_graph_backpropagates(spy):
    """the ``uses = 2`` pattern of test_gpu_glue_nodes.py: the second call refills the buffers the first call saved for backward (same
    bits, no version bump), and dW is the sum over the two uses"""
    m = _layer()
    xs = [[torch.randn(64, 96, device=dev()).requires_grad_(True) for _ in range(3)] for _ in range(2)]
    gs = [[torch.randn(64, 288, device=dev()) for _ in range(3)] for _ in range(2)]
    outs, gouts = [], []
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for x, xa, xb in xs:
            y, yt = m(x, {"a": xa, "b": xb})
            outs += [y, yt["a"], yt["b"]]
    for g3 in gs:
        gouts += [g.to(torch.bfloat16) for g in g3]
    torch.autograd.backward(outs, gouts)
    assert len(spy) == 2
    bf = lambda t: t.to(torch.bfloat16).double()
    ref = sum(sum(bf(g) for g in g3).t() @ bf(x3[0].detach()) for g3, x3 in zip(gs, xs))
    err = rel_err(m.linear.weight.grad, ref)
    print(f"layer used twice, linear.weight.grad: rel err {err:.3e}")
    assert err <= TOL[torch.bfloat16], err
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x3 in xs for x in x3)


# ----------------------------------------------------------------------------------------------
# the backbone of test_gpu_linear_bias.py with nothing frozen
# ----------------------------------------------------------------------------------------------
BB_TASKS = ["semseg", "normals"]


def _bb_cfg():
    return O.swin_t_cfg(img_size=56, tasks=BB_TASKS, r_shared=8, r_task=4, depths=(2, 2), num_heads=(3, 6), drop_path_rate=0.0, dropout=0.0)


def _bb_loss(stages, double):
    cast = (lambda t: t.double()) if double else (lambda t: t)
    return sum((s.to(torch.float64 if double else torch.float32) * cast(O.det_tensor(f"ba.g.{i}", s.shape, 1.0).to(s.device))).sum() +
               sum((tl[t].to(torch.float64 if double else torch.float32) * cast(O.det_tensor(f"ba.g.{i}.{t}", s.shape, 1.0).to(s.device))).sum()
                   for t in BB_TASKS) for i, (s, tl) in enumerate(stages))


@pytest.fixture(scope="module")
def backbone():
    """the backbone with every parameter trainable (FREEZE_PRETRAINED False) and the fp64 oracle's gradients, computed once"""
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerMTLoRA
    cfg = _bb_cfg()
    bb = SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                               window_size=7, drop_path_rate=0.0, tasks=BB_TASKS, mtlora=cfg["mtlora"])
    O.det_fill_(bb.named_parameters())
    bb = bb.to(dev()).train()
    x = O.det_tensor("fullft.x", (2, 3, 56, 56), 1.0).to(dev())
    trainable = {n for n, p in bb.named_parameters() if p.requires_grad}
    P = {k: v.detach().double().clone().requires_grad_(k in trainable) for k, v in bb.state_dict().items() if v.is_floating_point()}
    _bb_loss(O.backbone_stages(P, x.double(), cfg), True).backward()
    return bb, x, trainable, {n: P[n].grad for n in trainable}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16_autocast"])
def test_backbone_linear_weight_gradients_vs_oracle(backbone, spy, amp):
    """every ``*.linear.weight.grad`` of the 16 MTLoRALinear layers against the fp64 oracle: 2e-3 in fp32, 1e-2 under bf16 autocast"""
    bb, x, trainable, ref = backbone
    weights = sorted(n for n in trainable if n.endswith("linear.weight"))
    assert len(weights) == 16
    bb.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        got = bb(x, return_stages=True)
    _bb_loss(got, False).backward()
    assert len(spy) == 16
    named = dict(bb.named_parameters())
    worst = 0.0
    for n in weights:
        g = named[n].grad
        assert g is not None and g.dtype == torch.float32, n
        err = (g.double().cpu() - ref[n].cpu()).abs().max().item() / max(ref[n].abs().max().item(), 1e-9)
        worst = max(worst, err)
        print(f"backbone {n}.grad amp={amp}: rel err {err:.3e}")
        assert err <= (1e-2 if amp else 2e-3), (n, err)
    print(f"backbone linear.weight gradients amp={amp}: worst rel err {worst:.3e}")


# ----------------------------------------------------------------------------------------------
# the captured train step
# ----------------------------------------------------------------------------------------------
def test_graphed_train_step_full_fine_tuning():
    """GraphedTrainStep on the 56-px, depths (2, 2), two-task model built with freeze=False and the capturable HIP AdamW: three replays
    against three eager train_steps from the same state with the same dropout seeds and offsets.  Criterion, copied from
    test_gpu_optim_capturable.test_whole_step_graphed_with_scaler: losses and gradient norms within 2e-3 relative, cosine of the
    accumulated updates >= 0.98.  Every linear.weight has moved from its initial value (the replays re-read the masters)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    tasks = ["semseg", "normals"]
    img, tg = H.synthetic_batch(2, 56, tasks, seed=17, device=dev())
    kw = dict(img_size=56, tasks=tasks, depths=(2, 2), num_heads=(3, 6), r_shared=8, r_task=4, drop_path_rate=0.0, seed=4, freeze=False)
    out = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(**kw).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2)
            assert gs.graphed is True and gs.why == "", gs.why
            drawn = Fn._seed_counter  # two warm-up steps and the capture drew the layers' dropout seeds: three equal shares
            assert drawn % 3 == 0
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses, norms = [], []
            for _ in range(3):
                if use_graph:
                    loss, norm = gs(), gs.grad_norm
                else:  # the eager step, drawing the seeds the capture drew and walking the same device offset
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                    loss, norm = H.train_step(model, crit, opt, img, tg, clip_grad=5.0)
                losses.append(loss.clone())
                norms.append(norm.clone())
            torch.cuda.synchronize()
            moved = {n: (p.detach() - start[n]).double() for n, p in model.named_parameters() if n in start}
            out.append((losses, moved, norms))
            weights = [n for n in moved if n.endswith("linear.weight")]
            assert len(weights) == 16
            for n in weights:
                assert float(moved[n].abs().max()) > 0.0, f"{n} did not move ({'replay' if use_graph else 'eager'})"
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
