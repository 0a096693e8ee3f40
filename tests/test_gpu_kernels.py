"""GPU parity tests: the HIP path (through the C ABI / autograd Functions / modules) against the oracle and
the golden vectors captured from the reference.  Tolerances (BASELINE.json north_star): 1e-3 for fp32,
1e-2 for bf16, both relative to the output scale (max |ref|), since the reference's own bf16-vs-fp32
difference is 5e-3 relative."""
import ctypes

import math
import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2, torch.float16: 2e-3}  # fp16: 11-bit significand, fp32 accumulation


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _log_parity(what, err, tol, mult):
    """every measured error goes to gpurun_out/kernel_parity.jsonl (pulled back from the GPU box and committed as
    profiles/rNN_kernel_parity.jsonl): the record the tolerance multipliers below are set from"""
    import json
    import os
    try:
        os.makedirs("gpurun_out", exist_ok=True)
        with open("gpurun_out/kernel_parity.jsonl", "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what, "err": err,
                                "tol": tol, "mult": mult}) + "\n")
    except OSError:
        pass


def assert_close(a, b, dtype, what="", mult=1.0):
    e = rel_err(a, b)
    _log_parity(what, e, TOL[dtype], mult)
    assert e <= TOL[dtype] * mult, f"{what}: rel err {e:.3e} > {TOL[dtype] * mult:.1e}"


def eager_backbone_errors(cfg, x, dtype, c, tag, loss_tensors):
    """what the REFERENCE's own eager dataflow (the oracle's ATen ops under the same autocast dtype, on this GPU) loses against the
    fp64 fixture on the same 2-stage backbone: {parameter name: rel. gradient error}.  Stage outputs are held to the north-star
    tolerance (x1); a gradient behind four 16-bit blocks in a row to tolerance + the eager path's own error on that tensor,
    measured here -- never to a free multiplier."""
    P = {k: v.to(dev()).requires_grad_(True) for k, v in O.make_params(O.backbone_param_shapes(cfg)).items()}
    with torch.autocast("cuda", dtype=dtype):
        stages = O.backbone_stages(P, x, cfg)
    loss = 0
    for i, (st, tl) in enumerate(stages):
        loss = loss + (st.float() * O.det_tensor(f"{tag}.g.{i}", st.shape, 1.0).to(dev())).sum()
        for t in cfg["tasks"]:
            loss = loss + (tl[t].float() * O.det_tensor(f"{tag}.g.{i}.{t}", st.shape, 1.0).to(dev())).sum()
    loss.backward()
    errs = {}
    for n, g in c["grads"].items():
        if g is None or P[n].grad is None:
            continue
        got = P[n].grad.double().flatten().cpu()
        if isinstance(g, dict):
            scale = max(g["samples"].abs().max().item(), g.get("abssum", 0.0) / got.numel())
            errs[n] = ((got[g["idx"]] - g["samples"]).abs().max() / max(scale, 1e-12)).item()
        else:
            errs[n] = rel_err(P[n].grad, g)
    return errs


def grad_tol(dtype, eager, n):
    """north-star tolerance + the distance of the reference's own eager 16-bit result from the fp64 fixture on this tensor: what
    |hip - eager| <= tol (the north star's "match the reference PyTorch path within 1e-2 bf16") implies for the error against fp64"""
    return TOL[dtype] + eager.get(n, 0.0)


@pytest.fixture
def lowrank_form():
    """tests that aim at the kernels of the LOW-RANK form at ranks beyond min(K, N) (k_pq with 128-column tiles, rank strides of 256
    and more) switch lora.py's rank-aware association off: with it those shapes would run at rank min(K, N)"""
    from mtlora_amd import lora
    keep, lora.RANK_AWARE = lora.RANK_AWARE, False
    yield
    lora.RANK_AWARE = keep


# ------------------------------------------------------------------------------------------------
def test_library_loaded_and_layouts():
    """MFMA C/D layout and ds_read_b64_tr_b16 gather the kernels assume."""
    from mtlora_amd import _lib as L
    out = torch.zeros(4096, dtype=torch.int32, device=dev())
    L.check(L.lib().mtlora_selftest_layouts(L.ptr(out), L.stream_ptr()), "selftest")
    torch.cuda.synchronize()
    o = out.cpu()
    for base in (0, 1024):
        for lane in range(64):
            for r in range(16):
                row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
                col = lane & 31
                assert o[base + lane * 16 + r].item() == (row + 1) * (col + 1), (base, lane, r)
    for lane in range(64):
        for e in range(4):
            assert o[2048 + lane * 4 + e].item() == (lane & 15) + 16 * e + 64 * (lane >> 4), ("tr linear", lane, e)
    for lane in range(64):
        g, ig = lane >> 4, lane & 15
        for e in range(4):  # block base row 2g, cols 16(g&1)..+15 ; lane gets column ig, rows 0..3
            exp = (2 * g + e) * 72 + 16 * (g & 1) + ig
            assert o[2304 + lane * 4 + e].item() == exp, ("tr block", lane, e, o[2304 + lane * 4 + e].item(), exp)


# ------------------------------------------------------------------------------------------------
# window process
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sq", "rect", "noshift", "unit"])
def test_window_process_golden(golden, case):
    from mtlora_amd import window_process as WP
    c = golden("window_ops.pt")[case]
    B, H, W, C, ws, shift = c["dims"]
    x = c["x"].to(dev())
    got = WP.WindowProcess.apply(x, B, H, W, C, -shift, ws)
    assert torch.equal(got.cpu(), c["partitioned"])
    w = c["w"].to(dev())
    got = WP.WindowProcessReverse.apply(w, B, H, W, C, shift, ws)
    assert torch.equal(got.cpu(), c["merged"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_window_process_reference_unit_test_shape(dtype):
    """kernels/window_process/unit_test.py:123-195 (B=192, H=W=56, C=96, shift=2, ws=7), bit-exact,
    plus a REAL backward check (the reference's 'backward' tests compare forward outputs)."""
    from mtlora_amd import window_process as WP
    B, H, W, C, s, ws = 192, 56, 56, 96, 2, 7
    torch.manual_seed(0)
    x = torch.randn(B, H, W, C, device=dev()).to(dtype).requires_grad_(True)
    y = WP.WindowProcess.apply(x, B, H, W, C, -s, ws)
    exp = O.roll_and_window_partition(x.detach(), s, ws)
    assert torch.equal(y, exp)
    g = torch.randn_like(y)
    y.backward(g)
    assert torch.equal(x.grad, O.window_merge_and_roll(g, s, ws, H, W))
    w = torch.randn(B * (H // ws) * (W // ws), ws, ws, C, device=dev()).to(dtype).requires_grad_(True)
    z = WP.WindowProcessReverse.apply(w, B, H, W, C, s, ws)
    assert torch.equal(z, O.window_merge_and_roll(w.detach(), s, ws, H, W))
    g = torch.randn_like(z)
    z.backward(g)
    assert torch.equal(w.grad, O.roll_and_window_partition(g, s, ws))


def test_window_process_errors():
    from mtlora_amd import window_process as WP
    x = torch.randn(2, 14, 14, 8, device=dev())
    with pytest.raises(RuntimeError):
        WP.WindowProcess.apply(x.permute(0, 2, 1, 3), 2, 14, 14, 8, -3, 7)  # non-contiguous (CHECK_CONTIGUOUS)
    with pytest.raises(RuntimeError):
        WP.WindowProcess.apply(x.cpu(), 2, 14, 14, 8, -3, 7)  # CPU tensor (CHECK_CUDA)
    with pytest.raises(RuntimeError):
        WP.WindowProcess.apply(x, 2, 14, 14, 8, -3, 5)  # H % ws != 0


# ------------------------------------------------------------------------------------------------
# MTLoRALinear
# ------------------------------------------------------------------------------------------------
LINEAR_CASES = ["matrix_notasks", "matrix_tasks", "matrix_xtasks", "matrix_xtasks_nobias_r", "matrixv2_xtasks",
                "matrixv2_tasks", "addition_xtasks", "r0"]


def build_linear(c, dtype):
    from mtlora_amd.lora import MTLoRALinear
    K = c["params"]["linear.weight"].shape[1]
    N = c["params"]["linear.weight"].shape[0]
    m = MTLoRALinear(K, N, r=c["r"], lora_shared_scale=c["scale_s"], lora_task_scale=c["scale_t"], lora_dropout=0.0,
                     tasks=c["tasks"], shared_mode=c["mode"], bias=c["bias"])
    m.load_state_dict({k: v.float() for k, v in c["params"].items()})
    m.linear.weight.requires_grad_(False)
    if m.linear.bias is not None:
        m.linear.bias.requires_grad_(False)
    return m.to(dev())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", LINEAR_CASES)
def test_linear_golden(golden, case, dtype):
    c = golden("linear.pt")[case]
    m = build_linear(c, dtype)
    x = c["x"].to(dev()).to(dtype).requires_grad_(True)
    xt = {t: v.to(dev()).to(dtype).requires_grad_(True) for t, v in c["x_tasks"].items()} if c["x_tasks"] else None
    y, yt = m(x, xt)
    assert y.dtype == dtype
    assert_close(y, c["y"], dtype, "y")
    loss = (y.float() * c["gy"].to(dev()).float()).sum()
    if c["y_tasks"] is not None:
        for t in c["tasks"]:
            assert_close(yt[t], c["y_tasks"][t], dtype, f"y[{t}]")
            loss = loss + (yt[t].float() * c["gy_tasks"][t].to(dev()).float()).sum()
    else:
        assert yt is None
    loss.backward()
    assert_close(x.grad, c["dx"], dtype, "dx")
    if xt is not None:
        for t in c["tasks"]:
            assert_close(xt[t].grad, c["dx_tasks"][t], dtype, f"dx[{t}]")
    named = dict(m.named_parameters())
    for n, g in c["grads"].items():
        if n.startswith("linear."):
            assert named[n].grad is None  # frozen
            continue
        assert_close(named[n].grad, g, dtype, f"grad {n}")


def _oracle_linear(m, x, xt, keep=None, p=0.0):
    tasks = list(m.tasks) if (m.tasks is not None and m.r > 0) else None
    P = {k: v.detach().double().cpu().requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xs = x.detach().double().cpu().requires_grad_(True)
    xts = {t: v.detach().double().cpu().requires_grad_(True) for t, v in xt.items()} if xt else None
    y, yt = O.mtlora_linear(
        xs, P["linear.weight"], P.get("linear.bias"), P.get("lora_shared_A"), P.get("lora_shared_B"),
        m.lora_shared_scale if m.r > 0 else 0.0, tasks=tasks,
        A_t={t: P["lora_tasks_A." + t] for t in tasks} if tasks else None,
        B_t={t: P["lora_tasks_B." + t] for t in tasks} if tasks else None,
        scale_t=m.lora_task_scale if tasks else None, x_tasks=xts, shared_mode=m.shared_mode, keep_mask=keep, p=p)
    return P, xs, xts, y, yt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [
    # (M, K, N, r_s, r_t, T, x_tasks)   Swin-T stage shapes at reduced M, incl. ragged M and K % 32 != 0
    (1000, 96, 288, 64, 4, 0, False),     # qkv stage 0
    (777, 96, 384, 64, 4, 4, True),       # fc1 last block stage 0
    (520, 384, 96, 64, 4, 4, True),       # fc2 last block stage 0
    (300, 192, 192, 64, 4, 4, False),     # proj last block stage 1 (tasks read D(x))
    (260, 768, 3072, 64, 4, 0, False),    # fc1 stage 3
    (130, 3072, 768, 128, 128, 2, True),  # C4-like ranks
    (1, 96, 96, 16, 4, 1, True),          # single row
    # BASELINE configs[3]: Swin-B (C = 128 -> 1024), r = 128 shared and per task, 4 tasks
    (640, 128, 384, 128, 128, 4, True),   # qkv-like / fc1 stage 0 of Swin-B, R = 640 rank columns
    (384, 512, 128, 128, 128, 4, True),   # fc2 stage 0 of Swin-B
    (200, 1024, 1024, 128, 128, 4, False),  # proj stage 3 of Swin-B, tasks read D(x)
    # BASELINE configs[4]: 8 task heads, r swept over {4, 16, 64, 256}
    (500, 96, 384, 4, 4, 8, True),
    (500, 96, 384, 16, 16, 8, True),
    (333, 384, 96, 64, 64, 8, True),
    (260, 192, 192, 256, 256, 8, True),   # R = 9 * 256 rank columns
    (260, 96, 288, 256, 4, 8, False),
])
def test_linear_random_vs_oracle(shape, dtype):
    from mtlora_amd.lora import MTLoRALinear
    M, K, N, rs, rt, T, use_xt = shape
    tasks = [f"t{i}" for i in range(T)] or None
    torch.manual_seed(M + K)
    r = {"shared": rs, **{t: rt for t in (tasks or [])}}
    m = MTLoRALinear(K, N, r=r, lora_shared_scale=4.0, lora_task_scale={t: 4.0 for t in (tasks or [])} if tasks else 1.0,
                     lora_dropout=0.0, tasks=tasks).to(dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * (0.05 if "lora" in n else 0.02))
            if dtype != torch.float32:
                p.copy_(p.to(dtype).float())  # parameters exactly representable -> only accumulation order differs
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    x = torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True)
    xt = {t: torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True) for t in tasks} if (tasks and use_xt) else None
    y, yt = m(x, xt)
    P, xs, xts, yo, yto = _oracle_linear(m, x, xt)
    gy = torch.randn(M, N, device=dev()).to(dtype)
    assert_close(y, yo, dtype, "y")
    loss, loss_o = (y.float() * gy.float()).sum(), (yo * gy.double().cpu()).sum()
    gyt = {}
    for t in tasks or []:
        assert_close(yt[t], yto[t], dtype, f"y[{t}]")
        gyt[t] = torch.randn(M, N, device=dev()).to(dtype)
        loss = loss + (yt[t].float() * gyt[t].float()).sum()
        loss_o = loss_o + (yto[t] * gyt[t].double().cpu()).sum()
    loss.backward()
    loss_o.backward()
    assert_close(x.grad, xs.grad, dtype, "dx")
    for t in (tasks or []) if use_xt else []:
        assert_close(xt[t].grad, xts[t].grad, dtype, f"dx[{t}]")
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert_close(p.grad, P[n].grad, dtype, f"grad {n}")


@pytest.mark.parametrize("geom", [(333, 96, 160, torch.float32), (333, 96, 192, torch.bfloat16), (1100, 384, 96, torch.bfloat16),
                                  (500, 128, 256, torch.float16)])
@pytest.mark.parametrize("use_xt", [False, True])
def test_linear_dropout_matches_specified_generator(use_xt, geom):
    """train mode: the kernel's counter-based mask == oracle.dropout_keep_mask, forward and backward (fp32 on the tiled kernels;
    16-bit shapes that take the wave-streaming forward / dX / factor-gradient kernels, ragged M)."""
    from mtlora_amd.lora import MTLoRALinear
    from mtlora_amd import functional as Fn
    M, K, N, dtype = geom
    tasks = ["a", "b"]
    torch.manual_seed(3)
    m = MTLoRALinear(K, N, r={"shared": 16, "a": 4, "b": 8}, lora_shared_scale=2.0, lora_task_scale={"a": 3.0, "b": 1.5},
                     lora_dropout=0.25, tasks=tasks).to(dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * 0.05)
            if dtype != torch.float32:
                p.copy_(p.to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    x = torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True)
    xt = {t: torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True) for t in tasks} if use_xt else None
    seed_before = Fn._seed_counter
    y, yt = m(x, xt)
    # recover the seed the module drew
    Fn._seed_counter = seed_before
    seed = Fn.next_seed()
    keep = O.dropout_keep_mask(seed, 0, M, K, 0.25)
    frac = keep.float().mean().item()
    assert abs(frac - 0.75) < 0.01, frac
    P, xs, xts, yo, yto = _oracle_linear(m, x, xt, keep=keep, p=0.25)
    assert_close(y, yo, dtype, "y")
    loss, loss_o = y.float().sum() * 0.5, yo.sum() * 0.5
    for i, t in enumerate(tasks):
        assert_close(yt[t], yto[t], dtype, f"y[{t}]")
        loss, loss_o = loss + yt[t].float().sum() * (i + 1), loss_o + yto[t].sum() * (i + 1)
    loss.backward()
    loss_o.backward()
    assert_close(x.grad, xs.grad, dtype, "dx")
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert_close(p.grad, P[n].grad, dtype, f"grad {n}")
    m.eval()
    y2, _ = m(x, xt)
    P, xs, xts, yo2, _ = _oracle_linear(m, x, xt)
    assert_close(y2, yo2, dtype, "eval y")


def _t0_layer(K, N, r, dtype, p, scale=4.0):
    """a T = 0 MTLoRALinear in train mode whose parameters are exactly representable in ``dtype``"""
    from mtlora_amd.lora import MTLoRALinear
    m = MTLoRALinear(K, N, r={"shared": r}, lora_shared_scale=scale, lora_task_scale=1.0, lora_dropout=p, tasks=None).to(dev())
    with torch.no_grad():
        for n, q in m.named_parameters():
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n else 0.02))
            if dtype != torch.float32:
                q.copy_(q.to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    return m.train()


def _t0_train_case(m, M, dtype, p, kind, gdev, in_scale=1.0):
    """run one T = 0 layer in TRAIN mode through the HIP path (kind: None | "gelu_out" (fc1 of the Mlp) | "gate" (fc2 of the Mlp))
    and through the oracle in fp64 on ``gdev`` with the SPECIFIED dropout mask (oracle.dropout_keep_mask[_t] of the seed the module
    drew).  Returns dicts of HIP results and references: y, [a], dx (w.r.t. x, or w.r.t. h for "gate"), dA, dB."""
    from mtlora_amd import functional as Fn
    K, N = m.linear.in_features, m.linear.out_features
    c0 = Fn._seed_counter
    got, ref = {}, {}
    if kind == "gate":  # x = gelu(h); the layer's dX kernel multiplies by gelu'(h)
        h = (in_scale * 1.5 * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True)
        a = Fn.GeluDeferredGradFn.apply(h)
        y, _ = m(a, None, gelu_gate=(h, None))
        x_in, leaf = a.detach(), h
    else:
        x = (in_scale * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True)
        if kind == "gelu_out":
            y, _, a2, _ = m(x, None, gelu_out=True)
            got["a"] = a2
        else:
            y, _ = m(x, None)
        x_in, leaf = x.detach(), x
    Fn._seed_counter = c0
    seed = Fn.next_seed()
    gy = torch.randn(M, N, device=dev()).to(dtype)
    (y.float() * gy.float()).sum().backward()
    got.update(y=y, dx=leaf.grad, dA=m.lora_shared_A.grad, dB=m.lora_shared_B.grad)
    # ---- oracle, fp64 (ATen on gdev: the full-size cases take seconds there)
    keep = O.dropout_keep_mask_t(seed, 0, M, K, p, device=gdev)
    P = {k: v.detach().double().to(gdev).requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xo = x_in.double().to(gdev).requires_grad_(True)
    yo, _ = O.mtlora_linear(xo, P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                            keep_mask=keep, p=p)
    (yo * gy.double().to(gdev)).sum().backward()
    ref.update(y=yo.detach(), dx=xo.grad, dA=P["lora_shared_A"].grad, dB=P["lora_shared_B"].grad)
    if kind == "gelu_out":  # ATen semantics: gelu of the ROUNDED pre-activation
        ref["a"] = torch.nn.functional.gelu(y.detach().double().to(gdev))
    if kind == "gate":
        hd = leaf.detach().double().to(gdev).requires_grad_(True)
        torch.nn.functional.gelu(hd).backward(xo.grad)
        ref["dx"] = hd.grad
    return got, ref, keep


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("geom", [
    # (M, K, N, r_shared, r_task, T, x_tasks, p)
    (1500, 96, 288, 256, 0, 0, False, 0.1),     # T = 0, K < N: A' = I_96, B' = s B A -- the fused k_sp_xres / k_sp_ares at rank 96 instead of k_pq at 256
    (900, 384, 96, 256, 0, 0, False, 0.1),      # T = 0, K > N: A' = s B A, B' = I_96
    (700, 96, 384, 256, 256, 8, True, 0.05),    # c5:256 fc1T: 9 outputs, the tasks on their own inputs: 864 intermediate columns instead of 2304
    (700, 384, 96, 256, 256, 8, True, 0.05),    # c5:256 fc2T
    (500, 192, 192, 256, 256, 8, False, 0.05),  # c5:256 projT at stage 1: the tasks read D(x)
    (600, 96, 288, 64, 128, 2, True, 0.1),      # mixed: the shared update stays low-rank (64 < 96), the tasks' (128 > 96) do not
])
def test_linear_rank_aware_association_vs_oracle(geom, dtype):
    """lora.py's rank-aware association: an update of rank r > min(K, N) is applied as Delta W = s B A through
    the same library kernels (identity on one side), in TRAIN mode with the specified dropout mask -- outputs, dX, every dX_t and
    every factor gradient (formed by autograd from the N x K gradient the library returns) against the fp64 oracle, which evaluates
    the reference's low-rank formula (lora.py:253-284); the call must have gone out at rank min(K, N)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import lora
    M, K, N, r_s, r_t, nt, use_xt, p = geom
    tasks = _TASKS8[:nt] or None
    torch.manual_seed(M + K + nt)
    m = lora.MTLoRALinear(K, N, r={"shared": r_s, **{t: r_t for t in (tasks or [])}}, lora_shared_scale=2.0,
                          lora_task_scale={t: 1.5 for t in tasks} if tasks else 1.0, lora_dropout=p, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_((torch.randn_like(q) * (0.05 if "lora" in n_ else 0.02)).to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    xs_in = [(0.5 * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True) for _ in range(1 + (nt if use_xt else 0))]
    seen = []
    orig = Fn.MTLoRALinearFn.forward

    def spy(ctx, meta, *a):
        seen.append((meta.r_s, meta.r_t))
        return orig(ctx, meta, *a)

    Fn.MTLoRALinearFn.forward = staticmethod(spy)
    try:
        c0 = Fn._seed_counter
        y, yt = m(xs_in[0], {t: xs_in[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
        Fn._seed_counter = c0
        seed = Fn.next_seed()
    finally:
        Fn.MTLoRALinearFn.forward = staticmethod(orig)
    rm = min(K, N)
    assert seen == [(min(r_s, rm), tuple(min(r_t, rm) for _ in (tasks or [])))], seen
    outs = [y] + [yt[t] for t in (tasks or [])]
    gys = [torch.randn(M, N, device=dev()).to(dtype) for _ in outs]
    torch.autograd.backward(outs, gys)
    gdev = torch.device("cpu")
    keep = O.dropout_keep_mask_t(seed, 0, M, K, p, device=gdev)
    P = {k: v.detach().double().to(gdev).requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xo = [x.detach().double().to(gdev).requires_grad_(True) for x in xs_in]
    kw = {}
    if tasks:
        kw = dict(tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                  scale_t=m.lora_task_scale, x_tasks={t: xo[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
    yo, yto = O.mtlora_linear(xo[0], P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                              keep_mask=keep, p=p, **kw)
    refs = [yo] + [yto[t] for t in (tasks or [])]
    torch.autograd.backward(refs, [g.double().to(gdev) for g in gys])
    for i, (a, b) in enumerate(zip(outs, refs)):
        assert_close(a, b.detach(), dtype, f"y[{i}]")
    for i, (a, b) in enumerate(zip(xs_in, xo)):
        assert_close(a.grad, b.grad, dtype, f"dx[{i}]")
    for n_, q in m.named_parameters():
        if q.requires_grad:
            assert_close(q.grad, P[n_].grad, dtype, f"grad {n_}")


@pytest.mark.parametrize("geom", [
    # (M, K, N, dtype, kind): tasks=None -> the fused wave-streaming kernels of the 16-bit default path
    (333, 96, 288, torch.bfloat16, None),        # k_sp_xres forward (CH 96), k_sp_ares dX, ragged M
    (1100, 192, 576, torch.bfloat16, None),      # xres with two k-chunks and column parts; ares over 6 chunks, 2 parts
    (500, 128, 256, torch.float16, None),        # CH 64 forms, fp16
    (640, 64, 128, torch.float16, None),         # one 64-wide chunk
    (1000, 96, 96, torch.bfloat16, None),        # proj-like
    (300, 192, 768, torch.bfloat16, "gelu_out"),  # fc1 of the Mlp: GELU second output from the fused epilogue
    (777, 384, 96, torch.bfloat16, "gate"),      # fc2 of the Mlp: dX = k_sp_xres<GATE> (mask on the rank result, gelu' gate)
    (1100, 768, 192, torch.bfloat16, "gate"),    # fc2 stage 1
    (257, 96, 160, torch.float32, None),         # fp32: tiled kernels
])
def test_linear_dropout_t0_matches_specified_generator(geom):
    """train mode, layers WITHOUT tasks (36 of the 48 layers of a Swin-T step): the masks generated inside k_sp_xres (mask_act on the
    slab before the projection; dX form: mask_lr on the rank result) and k_sp_ares (mask_lr, per-chunk column offsets) -- or inside the
    tiled kernels in the [tiled] family -- equal oracle.dropout_keep_mask element for element: forward, dX and both factor
    gradients against the fp64 oracle evaluated with the specified mask (ADVICE r03 / VERDICT r03 weak 2)."""
    M, K, N, dtype, kind = geom
    p = 0.25
    torch.manual_seed(M + N)
    m = _t0_layer(K, N, 16 if K < 192 else 64, dtype, p, scale=2.0)
    got, ref, keep = _t0_train_case(m, M, dtype, p, kind, torch.device("cpu"))
    assert abs(keep.float().mean().item() - 0.75) < 0.01
    assert_close(got["y"], ref["y"], dtype, "y")
    if kind == "gelu_out":
        assert_close(got["a"], ref["a"], dtype, "gelu(y)")
    assert_close(got["dx"], ref["dx"], dtype, "dx")
    assert_close(got["dA"], ref["dA"], dtype, "dA")
    assert_close(got["dB"], ref["dB"], dtype, "dB")


def test_factor_side_stream_pending_paths():
    """functional._side_pending: (a) the SAME layer applied twice in one graph with the factor-gradient side stream
    installed -- the second call finds its factors pending from the first one in the same backward pass, waits for the side stream and
    keeps its own gradients on the main stream (autograd sums the two there); (b) the stream installed ONCE and two backward passes
    with nobody joining in between and the gradients accumulating into .grad; (c) after an un-joined pass whose gradients were
    dropped (zero_grad(set_to_none)), the side stream is used again.  Every variant must reproduce the single-stream gradients bit for
    bit (keyed by identity: the former WeakKeyDictionary compared Parameters with ``==`` and raised on the lookup)."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(3)
    dtype = torch.bfloat16
    m = _t0_layer(96, 96, 16, dtype, 0.0, scale=2.0)
    m2 = _t0_layer(96, 192, 16, dtype, 0.0, scale=2.0)
    x = (0.5 * torch.randn(9000, 96, device=dev())).to(dtype)
    keep_m = Fn._FACTOR_MIN_M
    side = torch.cuda.Stream()

    def grads():
        return [q.grad.detach().clone() for mod in (m, m2) for q in (mod.lora_shared_A, mod.lora_shared_B)]

    def run(passes, use_side, zero_between=False):
        for mod in (m, m2):
            mod.zero_grad(set_to_none=True)
        Fn.factor_stream_joined()
        Fn.set_factor_stream(side if use_side else None)
        marked = 0
        try:
            for i in range(passes):
                xi = x.clone().requires_grad_(True)
                y, _ = m(xi)
                y, _ = m(y)            # the same layer a second time in the same graph
                z, _ = m2(y)
                (z.float() ** 2).mean().backward()
                marked = max(marked, len(Fn._side_pending))
                if zero_between and i + 1 < passes:
                    torch.cuda.current_stream().wait_stream(side)
                    for mod in (m, m2):
                        mod.zero_grad(set_to_none=True)
        finally:
            Fn.set_factor_stream(None)
        torch.cuda.current_stream().wait_stream(side)
        Fn.factor_stream_joined()
        torch.cuda.synchronize()
        return grads(), marked

    try:
        Fn._FACTOR_MIN_M = 0
        ref1, n0 = run(1, False)
        got1, n1 = run(1, True)
        assert n0 == 0 and n1 == 4  # pending at the end of the pass: m2's two factors and m's (re-marked under the current pass: round 6)
        ref2, _ = run(2, False)
        got2, _ = run(2, True)
        got3, n3 = run(2, True, zero_between=True)
        ref3, _ = run(1, False)
    finally:
        Fn._FACTOR_MIN_M = keep_m
    for a, b in zip(ref1 + ref2 + ref3, got1 + got2 + got3):
        assert torch.equal(a, b)
    assert n3 == 4


def test_factor_side_stream_three_uses_and_tensor_hooks():
    """(a) the same layer THREE times in one graph -- the second use pops the entry of the first; unless it is put back the
    third use goes to the side stream again and autograd sums it with the first two on the main stream without waiting; (b) a tensor
    hook on a factor Parameter receives the gradient on the backward's stream, so that layer must keep its factor gradients there.
    Both must reproduce the single-stream gradients bit for bit, and (b) must not have marked the hooked layer's factors."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(4)
    dtype = torch.bfloat16
    m = _t0_layer(96, 96, 16, dtype, 0.0, scale=2.0)
    x = (0.5 * torch.randn(9000, 96, device=dev())).to(dtype)
    keep_m = Fn._FACTOR_MIN_M
    side = torch.cuda.Stream()
    seen = []

    def run(use_side, hook=False):
        m.zero_grad(set_to_none=True)
        Fn.factor_stream_joined()
        Fn.set_factor_stream(side if use_side else None)
        h = m.lora_shared_A.register_hook(lambda g: seen.append(float(g.float().abs().sum())) or g * 1.0) if hook else None
        try:
            xi = x.clone().requires_grad_(True)
            y, _ = m(xi)
            y, _ = m(y)
            y, _ = m(y)   # third use in the same graph
            (y.float() ** 2).mean().backward()
            marked = len(Fn._side_pending)
        finally:
            Fn.set_factor_stream(None)
            if h is not None:
                h.remove()
        torch.cuda.current_stream().wait_stream(side)
        Fn.factor_stream_joined()
        torch.cuda.synchronize()
        return [m.lora_shared_A.grad.detach().clone(), m.lora_shared_B.grad.detach().clone()], marked

    try:
        Fn._FACTOR_MIN_M = 0
        ref, _ = run(False)
        got, n = run(True)
        ref_h, _ = run(False, hook=True)
        got_h, n_h = run(True, hook=True)
    finally:
        Fn._FACTOR_MIN_M = keep_m
    assert n == 2 and n_h == 0
    for a, b in zip(ref + ref_h, got + got_h):
        assert torch.equal(a, b)


def test_linear_unused_output_gets_none_grad():
    """final stage: the shared output is never consumed -> lora_shared_{A,B} must get NO gradient."""
    from mtlora_amd.lora import MTLoRALinear
    m = MTLoRALinear(96, 96, r={"shared": 8, "a": 4}, lora_shared_scale=1.0, lora_task_scale={"a": 1.0}, tasks=["a"]).to(dev())
    with torch.no_grad():
        m.lora_shared_B.normal_()
        m.lora_tasks_B["a"].normal_()
    x = torch.randn(50, 96, device=dev(), requires_grad=True)
    y, yt = m(x)
    yt["a"].sum().backward()
    assert m.lora_shared_A.grad is None and m.lora_shared_B.grad is None
    assert m.lora_tasks_A["a"].grad is not None and x.grad is not None


def test_linear_errors():
    from mtlora_amd.lora import MTLoRALinear
    m = MTLoRALinear(96, 96, r=4)
    with pytest.raises(RuntimeError):
        m(torch.randn(4, 96))  # CPU tensor: no fallback
    m = MTLoRALinear(96, 98, r=4).to(dev())  # N % 4 != 0
    with pytest.raises(RuntimeError):
        m(torch.randn(4, 96, device=dev()))


def test_merge_matches_unmerged_eval():
    """MTLoRALinear.merge() / checkpoint.merge_lora_weights: a 2-stage backbone in eval mode gives the same stage outputs
    before and after folding W' = W + s B A into every mergeable layer (all layers without tasks), and unmerge restores
    the weights bit for bit... up to the fp32 rounding of the add/sub pair."""
    from mtlora_amd.checkpoint import merge_lora_weights, unmerge_lora_weights
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerMTLoRA
    tasks = ["semseg", "normals"]
    cfg = O.swin_t_cfg(img_size=56, tasks=tasks, r_shared=8, r_task=4, depths=(2, 2), num_heads=(3, 6), drop_path_rate=0.1, dropout=0.05)
    bb = SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                               window_size=7, drop_path_rate=0.1, tasks=tasks, mtlora=cfg["mtlora"])
    O.det_fill_(bb.named_parameters())
    bb = bb.to(dev()).eval()
    x = O.det_tensor("merge.x", (2, 3, 56, 56), 1.0).to(dev())
    w_before = {n: p.detach().clone() for n, p in bb.named_parameters() if n.endswith("linear.weight")}
    with torch.no_grad():
        ref = bb(x, return_stages=True)
        n = merge_lora_weights(bb)
        assert n == 2 * 2 * 4 - 2 * 3   # 16 linears, the 3 task-enabled ones of each stage's last block stay unmerged
        got = bb(x, return_stages=True)
        for (s, tl), (rs, rtl) in zip(got, ref):
            assert_close(s, rs, torch.float32, "merged stage output")
            for t in tasks:
                assert_close(tl[t], rtl[t], torch.float32, f"merged task output {t}")
        assert unmerge_lora_weights(bb) == n
    for k, w in w_before.items():
        assert torch.allclose(dict(bb.named_parameters())[k], w, atol=1e-6), k


# ------------------------------------------------------------------------------------------------
# window attention
# ------------------------------------------------------------------------------------------------
def _regions(H, W, ws, shift):
    """region ids of the SW-MSA mask, derived from the ORACLE's dense mask: ids differ <=> mask == -100."""
    from mtlora_amd.swin_transformer_mtlora import _shift_regions
    ids = _shift_regions(H, W, ws, shift).to(torch.int32)
    dense = O.shifted_window_mask(H, W, ws, shift)
    rebuilt = torch.where(ids[:, None, :] != ids[:, :, None], torch.tensor(-100.0), torch.tensor(0.0))
    assert torch.equal(rebuilt, dense)
    return ids


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [
    # (B, H, W, heads, ws, shift)
    (2, 14, 14, 3, 7, 3), (2, 14, 14, 3, 7, 0), (1, 14, 21, 2, 7, 2), (3, 7, 7, 6, 7, 0), (2, 8, 8, 1, 4, 2),
    (1, 16, 16, 2, 8, 3),
])
def test_attention_core_vs_oracle(cfg, dtype):
    """both layouts: image (shift folded into addressing) and windows (reference module API)."""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = cfg
    C, N = nH * 32, ws * ws
    torch.manual_seed(H * W + nH)
    qkv_img = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype).requires_grad_(True)
    bias = (torch.randn(nH, N, N, device=dev()) * 0.5).requires_grad_(True)
    mask = O.shifted_window_mask(H, W, ws, shift)
    mask_d = None if mask is None else mask.to(dev())
    scale = 32 ** -0.5
    meta = Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=scale)
    ids = None if mask is None else _regions(H, W, ws, shift).to(dev())
    out = Fn.WindowAttentionFn.apply(meta, qkv_img, bias, None, ids)          # region-id fast path
    # oracle: roll + partition -> core -> merge + roll
    q64 = qkv_img.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True)
    win = O.roll_and_window_partition(q64, shift, ws).reshape(-1, N, 3 * C)
    core = O.window_attention_core(win, b64, None if mask is None else mask.double(), nH, scale)
    ref = O.window_merge_and_roll(core.reshape(-1, ws, ws, C), shift, ws, H, W)
    assert_close(out, ref, dtype, "attn out")
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double().cpu())
    assert_close(qkv_img.grad, q64.grad, dtype, "dqkv")
    assert_close(bias.grad, b64.grad, dtype, "dbias")
    # window-major layout
    qkv_win = win.detach().to(dev()).to(dtype).contiguous().requires_grad_(True)
    nW = 1 if mask is None else mask.shape[0]
    meta_w = Fn.AttnMeta(B=qkv_win.shape[0] // nW, H=ws, W=ws * nW, window_size=ws, shift=0, num_heads=nH, head_dim=32,
                         image_layout=False, scale=scale)
    out_w = Fn.WindowAttentionFn.apply(meta_w, qkv_win, bias.detach(), mask_d, None)   # general dense-mask path
    assert_close(out_w, core, dtype, "attn out (windows)")
    if mask is not None:  # dense-mask path, image layout, forward + backward
        q2 = qkv_img.detach().clone().requires_grad_(True)
        b2 = bias.detach().clone().requires_grad_(True)
        out_d = Fn.WindowAttentionFn.apply(meta, q2, b2, mask_d, None)
        assert_close(out_d, ref, dtype, "attn out (dense mask)")
        out_d.backward(g)
        assert_close(q2.grad, q64.grad, dtype, "dqkv (dense mask)")
        assert_close(b2.grad, b64.grad, dtype, "dbias (dense mask)")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attention_large_relative_bias_vs_oracle(dtype):
    """relative-position bias of TRAINED magnitude (|bias| up to ~15; random init is 0.02): the 16-bit kernels feed bias / scale through
    the matrix pipe in the compute type (csrc/attention.hip, BiasSrc), i.e. each bias term carries a 2^-9 relative rounding that an fp32
    add would not.  Pinned here at the north-star tolerance against the fp64 oracle, forward, dqkv and dbias -- next to
    the reference's own eager bf16-autocast arithmetic (q k^T rounded to bf16 before the fp32 bias is added,
    swin_transformer_mtlora.py:200-207), whose error against the same fp64 values must not be smaller by more than 4x (or the HIP
    error stays under half the tolerance).  Round 5: the bias product is an fp16 MFMA in the bf16 kernels too -- as a bf16 operand this
    test read 1.3e-2 forward error in bf16."""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = 2, 14, 14, 3, 7, 3
    C, N = nH * 32, ws * ws
    torch.manual_seed(77)
    qkv = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype).requires_grad_(True)
    bias = (torch.randn(nH, N, N, device=dev()) * 5.0).requires_grad_(True)
    mask = O.shifted_window_mask(H, W, ws, shift)
    scale = 32 ** -0.5
    meta = Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=scale)
    out = Fn.WindowAttentionFn.apply(meta, qkv, bias, None, _regions(H, W, ws, shift).to(dev()))
    g = torch.randn_like(out)
    out.backward(g)
    q64 = qkv.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True)
    win = O.roll_and_window_partition(q64, shift, ws).reshape(-1, N, 3 * C)
    ref = O.window_merge_and_roll(O.window_attention_core(win, b64, mask.double(), nH, scale).reshape(-1, ws, ws, C), shift, ws, H, W)
    ref.backward(g.double().cpu())
    assert bias.detach().abs().max().item() > 12.0
    assert_close(out, ref, dtype, "attn out, |bias| ~ 5")
    assert_close(qkv.grad, q64.grad, dtype, "dqkv, |bias| ~ 5")
    assert_close(bias.grad, b64.grad, dtype, "dbias, |bias| ~ 5")
    # the reference's eager dataflow under autocast on the same inputs (oracle ops through ATen on the GPU)
    qe = qkv.detach().float().requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        wine = O.roll_and_window_partition(qe, shift, ws).reshape(-1, N, 3 * C)
        eag = O.window_merge_and_roll(O.window_attention_core(wine, bias.detach(), mask.to(dev()), nH, scale).reshape(-1, ws, ws, C),
                                      shift, ws, H, W)
    e_hip, e_eager = rel_err(out, ref), rel_err(eag.float(), ref)
    _log_parity("attn out |bias|~5: eager autocast error", e_eager, TOL[dtype], 1.0)
    _log_parity("attn out |bias|~5: hip error", e_hip, TOL[dtype], 1.0)
    assert e_hip <= max(4.0 * e_eager, 0.5 * TOL[dtype]), (e_hip, e_eager)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["nomask", "mask"])
def test_window_attention_module_golden(golden, case, dtype):
    from mtlora_amd.swin_transformer_mtlora import WindowAttention
    c = golden("window_attention.pt")[case]
    mt = O.mtlora_config(c["tasks"], r_shared=8, r_task=4, dropout=0.0)
    att = WindowAttention(64, (7, 7), c["heads"], lora=c["lora"], tasks=c["tasks"], mtlora=mt, layer_idx=0)
    att.load_state_dict({**{k: v.float() for k, v in c["params"].items()}, "relative_position_index": c["rel_index"]})
    att = att.to(dev()).eval()
    x = c["x"].to(dev()).to(dtype).requires_grad_(True)
    mask = None if c["mask"] is None else c["mask"].float().to(dev())
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if dtype == torch.bfloat16 else torch.autocast("cuda", enabled=False)
    with ctx:
        y, yt = att(x, mask)
    assert_close(y, c["y"], dtype, "y")
    loss = (y.float() * O.det_tensor(f"att.{case}.gy", y.shape, 1.0).to(dev())).sum()
    if c["y_tasks"]:
        for t in c["tasks"]:
            assert_close(yt[t], c["y_tasks"][t], dtype, f"y[{t}]")
            loss = loss + (yt[t].float() * O.det_tensor(f"att.{case}.gy.{t}", y.shape, 1.0).to(dev())).sum()
    loss.backward()
    assert_close(x.grad, c["dx"], dtype, "dx")
    named = dict(att.named_parameters())
    for n, g in c["grads"].items():
        assert_close(named[n].grad, g, dtype, f"grad {n}")


# ------------------------------------------------------------------------------------------------
# block / backbone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["image", "windows"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", ["shift_lora", "noshift_plain"])
def test_swin_block_golden(golden, case, dtype, layout):
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerBlock
    c = golden("swin_block.pt")[case]
    tasks = c["tasks"]
    mt = O.mtlora_config(tasks, r_shared=8, r_task=4, dropout=0.0)
    blk = SwinTransformerBlock(64, (14, 14), 2, window_size=7, shift_size=c["shift"], lora=c["lora"], tasks=tasks,
                               mtlora=mt, layer_idx=0, drop_path=0.1)
    O.det_fill_(blk.named_parameters())
    blk = blk.to(dev()).eval()
    blk.attention_layout = layout
    x = c["x"].to(dev()).float().requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        y, yt = blk(x)
    assert_close(y, c["y"], dtype, "y")
    loss = (y.float() * O.det_tensor(f"blk.{case}.gy", y.shape, 1.0).to(dev())).sum()
    if c["y_tasks"]:
        for t in tasks:
            assert_close(yt[t], c["y_tasks"][t], dtype, f"y[{t}]")
            loss = loss + (yt[t].float() * O.det_tensor(f"blk.{case}.gy.{t}", y.shape, 1.0).to(dev())).sum()
    else:
        assert yt is None
    loss.backward()
    assert_close(x.grad, c["dx"], dtype, "dx")
    named = dict(blk.named_parameters())
    for n, g in c["grads"].items():
        if isinstance(g, dict):
            s = named[n].grad.double().flatten().cpu()
            ref = g["samples"]
            assert ((s[g["idx"]] - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item() <= TOL[dtype] * 3, n
        else:
            assert_close(named[n].grad, g, dtype, f"grad {n}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_backbone_small_golden(golden, dtype):
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerMTLoRA
    c = golden("backbone_small.pt")
    tasks = c["tasks"]
    cfg = O.swin_t_cfg(img_size=56, tasks=tasks, r_shared=8, r_task=4, depths=(2, 2), num_heads=(3, 6),
                       drop_path_rate=0.1, dropout=0.05)
    bb = SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2],
                               num_heads=[3, 6], window_size=7, drop_path_rate=0.1, tasks=tasks, mtlora=cfg["mtlora"])
    assert list(bb.state_dict().keys()) == c["names"]
    O.det_fill_(bb.named_parameters())
    bb = bb.to(dev()).eval()
    x = O.det_tensor("bbs.x", (1, 3, 56, 56), 1.0).to(dev())
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        stages = bb(x, return_stages=True)
    loss = 0
    for i, (s, tl) in enumerate(stages):
        assert_close(s, c["stages"][i][0], dtype, f"stage {i}")
        loss = loss + (s.float() * O.det_tensor(f"bbs.g.{i}", s.shape, 1.0).to(dev())).sum()
        for t in tasks:
            assert_close(tl[t], c["stages"][i][1][t], dtype, f"stage {i} {t}")
            loss = loss + (tl[t].float() * O.det_tensor(f"bbs.g.{i}.{t}", s.shape, 1.0).to(dev())).sum()
    loss.backward()
    named = dict(bb.named_parameters())
    # gradients: the north-star tolerance + what the reference's own eager 16-bit dataflow loses on that tensor (grad_tol)
    eager = eager_backbone_errors(cfg, x, dtype, c, "bbs", None) if dtype != torch.float32 else {}
    for n, g in c["grads"].items():
        if g is None:
            assert named[n].grad is None, n
        elif isinstance(g, dict):
            s = named[n].grad.double().flatten().cpu()
            ref = g["samples"]
            e = ((s[g["idx"]] - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()
            _log_parity(f"grad {n} (samples; eager {eager.get(n, 0.0):.2e})", e, TOL[dtype], grad_tol(dtype, eager, n) / TOL[dtype])
            assert e <= grad_tol(dtype, eager, n), (n, e, eager.get(n))
        else:
            assert_close(named[n].grad, g, dtype, f"grad {n} (eager {eager.get(n, 0.0):.2e})", mult=grad_tol(dtype, eager, n) / TOL[dtype])
    assert sorted(n for n, p in bb.named_parameters() if p.grad is None) == c["grad_is_none"]


# ------------------------------------------------------------------------------------------------
# LayerNorm glue kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["downsampler", "intermediate", "trainable_scale"])
def test_backbone_options_golden(golden, case, dtype):
    """the non-default MTLoRA switches of the shipped yamls through the HIP path vs fixtures from the real reference:
    DOWNSAMPLER_ENABLED (mtlora_plus_*: the PatchMerging reduction is an MTLoRALinear over the stacked streams),
    INTERMEDIATE_SPECIALIZATION (every block emits task outputs; only the last one's survive), TRAINABLE_SCALE_SHARED (the
    scale is a Parameter: its gradient <dB, B> / s and the same trainable set)."""
    from mtlora_amd.lora import mark_only_lora_as_trainable
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerMTLoRA
    c = golden("backbone_options.pt")[case]
    tasks = c["tasks"]
    cfg = O.swin_t_cfg(img_size=56, tasks=tasks, r_shared=8, r_task=4, depths=(2, 2), num_heads=(3, 6), drop_path_rate=0.1,
                       dropout=0.05, **c["over"])
    bb = SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                               window_size=7, drop_path_rate=0.1, tasks=tasks, mtlora=cfg["mtlora"])
    assert [n for n in bb.state_dict().keys()] == c["names"]
    O.det_fill_(bb.named_parameters())
    mark_only_lora_as_trainable(bb, bias="none")
    assert [n for n, p in bb.named_parameters() if p.requires_grad] == c["trainable"]
    bb = bb.to(dev()).eval()
    x = O.det_tensor("bbo.x", (1, 3, 56, 56), 1.0).to(dev())
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        stages = bb(x, return_stages=True)
    loss = 0
    for i, (s, tl) in enumerate(stages):
        assert_close(s, c["stages"][i][0], dtype, f"stage {i}")
        loss = loss + (s.float() * O.det_tensor(f"bbo.g.{i}", s.shape, 1.0).to(dev())).sum()
        for t in tasks:
            assert_close(tl[t], c["stages"][i][1][t], dtype, f"stage {i} {t}")
            loss = loss + (tl[t].float() * O.det_tensor(f"bbo.g.{i}.{t}", s.shape, 1.0).to(dev())).sum()
    loss.backward()
    named = dict(bb.named_parameters())
    # gradients: the north-star tolerance + what the reference's own eager bf16 dataflow loses on that tensor (grad_tol; measured
    # here, on the same fixture); fp32: the scale gradients -- ONE scalar each, an inner product of two near-zero-mean tensors -- keep 3e-3
    eager = eager_backbone_errors(cfg, x, dtype, c, "bbo", None) if dtype != torch.float32 else {}
    scale_grads, scale_eager = [], []
    for n, g in c["grads"].items():
        got = named[n].grad
        assert got is not None, n
        if isinstance(g, dict):
            f = got.double().flatten().cpu()
            scale = max(g["samples"].abs().max().item(), g["abssum"] / f.numel())
            e = (f[g["idx"]] - g["samples"]).abs().max().item() / scale
            _log_parity(f"{n} (samples; eager {eager.get(n, 0.0):.2e})", e, TOL[dtype], grad_tol(dtype, eager, n) / TOL[dtype])
            assert e <= grad_tol(dtype, eager, n), (n, e, eager.get(n))
        elif n.endswith("lora_shared_scale") and dtype == torch.bfloat16:
            scale_grads.append((got.detach().float().cpu().reshape(1), g.float().reshape(1)))
            scale_eager.append(eager.get(n, 0.0) * g.abs().item())
        elif n.endswith("lora_shared_scale"):
            assert_close(got, g, dtype, n, mult=3)
        else:
            assert_close(got, g, dtype, f"{n} (eager {eager.get(n, 0.0):.2e})", mult=grad_tol(dtype, eager, n) / TOL[dtype])
    if scale_grads:
        # bf16: the 16 scale scalars are compared as one vector, relative to its largest entry -- tolerance + the eager bf16 path's
        # error on the same vector
        ref_v = torch.cat([b for _, b in scale_grads])
        ev = max(scale_eager) / ref_v.abs().max().item()
        assert_close(torch.cat([a for a, _ in scale_grads]), ref_v, dtype, f"scale grads (eager {ev:.2e})", mult=1.0 + ev / TOL[dtype])
    assert sorted(n for n in c["trainable"] if named[n].grad is None or named[n].grad.abs().max() == 0) == c["grad_is_none"]


@pytest.mark.parametrize("xdt,ydt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                     (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16), (torch.float16, torch.float16)])
@pytest.mark.parametrize("M,C", [(1000, 96), (333, 192), (257, 384), (100, 768), (65, 1536), (3, 2048), (50, 40)])
def test_layernorm_vs_torch(M, C, xdt, ydt):
    from mtlora_amd import functional as Fn
    torch.manual_seed(M + C)
    x = (torch.randn(M, C, device=dev()) * 2 + 0.5).to(xdt).requires_grad_(True)
    w = (torch.randn(C, device=dev()) * 0.2 + 1).requires_grad_(True)
    b = (torch.randn(C, device=dev()) * 0.1).requires_grad_(True)
    y = Fn.LayerNormFn.apply(x, w, b, 1e-5, ydt)
    assert y.dtype == ydt
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64, b64 = w.detach().double().cpu().requires_grad_(True), b.detach().double().cpu().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(x64, (C,), w64, b64, 1e-5)
    assert_close(y, ref, ydt, "y")
    g = torch.randn(M, C, device=dev()).to(ydt)
    y.backward(g)
    ref.backward(g.double().cpu())
    assert_close(x.grad, x64.grad, xdt, "dx")
    assert_close(w.grad, w64.grad, ydt, "dgamma")
    assert_close(b.grad, b64.grad, ydt, "dbeta")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R,C,relu", [(5000, 1080, True), (777, 1080, False), (4096, 64, True), (100, 8, True)])
def test_batchnorm_relu_vs_torch(R, C, relu, dtype):
    from mtlora_amd import functional as Fn
    torch.manual_seed(R + C)
    x = (torch.randn(R, C, device=dev()) * 1.5 + 0.3).to(dtype).requires_grad_(True)
    w = (torch.randn(C, device=dev()) * 0.2 + 1).requires_grad_(True)
    b = (torch.randn(C, device=dev()) * 0.3).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
    y = Fn.BatchNormReluFn.apply(x, w, b, rm, rv, 0.1, 1e-5, relu)
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64, b64 = w.detach().double().cpu().requires_grad_(True), b.detach().double().cpu().requires_grad_(True)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    ref = torch.nn.functional.batch_norm(x64, rm64, rv64, w64, b64, True, 0.1, 1e-5)
    if relu:
        ref = torch.relu(ref)
    assert_close(y, ref, dtype, "y")
    assert_close(rm, rm64, torch.float32, "running_mean")
    assert_close(rv, rv64, torch.float32, "running_var")
    g = torch.randn(R, C, device=dev()).to(dtype)
    y.backward(g)
    ref.backward(g.double().cpu())
    assert_close(x.grad, x64.grad, dtype, "dx")
    assert_close(w.grad, w64.grad, dtype, "dgamma")
    assert_close(b.grad, b64.grad, dtype, "dbeta")


@pytest.mark.parametrize("rdt,ydt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32),
                                     (torch.float32, torch.float16)])
@pytest.mark.parametrize("shared", [True, False])
def test_residual_droppath(shared, rdt, ydt):
    from mtlora_amd import functional as Fn
    torch.manual_seed(5)
    B, Ltok, C, n = 6, 49, 96, 3
    res = [torch.randn(B, Ltok, C, device=dev()).to(rdt).requires_grad_(True) for _ in range(1 if shared else n)]
    ys = [torch.randn(B, Ltok, C, device=dev()).to(ydt).requires_grad_(True) for _ in range(n)]
    scale = (torch.rand(n, B, device=dev()) < 0.7).float() / 0.7
    outs = Fn.ResidualDropPathFn.apply(scale, shared, n, *res, *ys)
    gs = [torch.randn_like(o) for o in outs]
    torch.autograd.backward([outs[0], outs[2]], [gs[0], gs[2]])     # output 1 gets no gradient
    r64 = [r.detach().double().requires_grad_(True) for r in res]
    y64 = [y.detach().double().requires_grad_(True) for y in ys]
    ref = [(r64[0] if shared else r64[k]) + scale[k].double().view(B, 1, 1) * y64[k] for k in range(n)]
    torch.autograd.backward([ref[0], ref[2]], [gs[0].double(), gs[2].double()])
    for k in range(n):
        assert outs[k].dtype == rdt
        assert_close(outs[k], ref[k], rdt, f"out{k}")
    for a, b in zip(res, r64):
        if b.grad is None:
            assert a.grad is None
        else:
            assert_close(a.grad, b.grad, rdt, "dres")
    for k in (0, 2):
        assert_close(ys[k].grad, y64[k].grad, ydt, f"dy{k}")
    assert ys[1].grad is None


_ULP = {torch.float32: 2.0 ** -23, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_SEVEN_PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float32),
                (torch.float16, torch.float16), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                (torch.bfloat16, torch.bfloat16)]


@pytest.mark.parametrize("rdt,ydt", _SEVEN_PAIRS)
def test_residual_droppath_every_dtype_pair(rdt, ydt):
    """mtlora_residual_droppath_fwd / _bwd called directly for each of the seven (res, y) dtype pairs of the host ladder, at the
    smallest shape (n = 2, B = 2, M = 64, C = 8), against the same formula in fp64 on the rounded inputs.  One multiply-add per element:
    the result is within one unit in the last place of its dtype of the exact value, taken relative to the result and to the
    scale * y term (the sum of the gradients for dres); a swapped branch of the ladder reads the wrong element size and is off by
    order one."""
    from mtlora_amd import _lib
    n, B, M, C = 2, 2, 64, 8
    torch.manual_seed(11)
    res = [torch.randn(M, C, device=dev()).to(rdt) for _ in range(n)]
    ys = [torch.randn(M, C, device=dev()).to(ydt) for _ in range(n)]
    scale = ((torch.rand(n, B, device=dev()) < 0.7).float() / 0.7).contiguous()
    scale[0, 0] = 1.0 / 0.7  # (at least one kept sample)
    outs = [torch.full((M, C), float("nan"), device=dev(), dtype=rdt) for _ in range(n)]
    L, P9 = _lib.lib(), _lib.ptr_array9
    rc, yc = _lib.dtype_code(res[0]), _lib.dtype_code(ys[0])
    _lib.check(L.mtlora_residual_droppath_fwd(n, P9(res), P9(ys), P9(outs), _lib.ptr(scale), M, C, B, rc, yc, _lib.stream_ptr()), "fwd")
    s64 = scale.double().repeat_interleave(M // B, dim=1).unsqueeze(-1)  # (n, M, 1)
    for k in range(n):
        term = s64[k] * ys[k].double()
        ref = res[k].double() + term
        err = (outs[k].double() - ref).abs()
        assert (err <= _ULP[rdt] * (ref.abs() + term.abs())).all(), (k, err.max().item())
    gs = [torch.randn(M, C, device=dev()).to(rdt) for _ in range(n)]
    dys = [torch.full((M, C), float("nan"), device=dev(), dtype=ydt) for _ in range(n)]
    dres = torch.full((M, C), float("nan"), device=dev(), dtype=rdt)
    _lib.check(L.mtlora_residual_droppath_bwd(n, P9(gs), P9(dys), _lib.ptr(dres), _lib.ptr(scale), M, C, B, rc, yc, _lib.stream_ptr()), "bwd")
    for k in range(n):
        ref = s64[k] * gs[k].double()
        assert ((dys[k].double() - ref).abs() <= 2 * _ULP[ydt] * ref.abs()).all(), k
    ref = sum(g.double() for g in gs)
    assert ((dres.double() - ref).abs() <= _ULP[rdt] * (ref.abs() + sum(g.double().abs() for g in gs))).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_upsample_cl_every_dtype(dtype):
    """mtlora_upsample_cl_fwd / _bwd called directly for each dtype of the host ladder at the smallest shape (B = 1, h = w = 2,
    C = 4, scale 2) against F.interpolate(bilinear) and its transpose in fp64 on the rounded inputs; tolerance of
    test_concat_upsample_vs_torch for the dtype."""
    from mtlora_amd import _lib
    B, h, w, C, S = 1, 2, 2, 4, 2
    torch.manual_seed(3)
    coarse = torch.randn(B, h, w, C, device=dev()).to(dtype)
    fine = torch.full((B, h * S, w * S, C), float("nan"), device=dev(), dtype=dtype)
    L, code = _lib.lib(), _lib.dtype_code(coarse)
    _lib.check(L.mtlora_upsample_cl_fwd(_lib.ptr(coarse), _lib.ptr(fine), B, h, w, C, S, C, code, _lib.stream_ptr()), "fwd")
    c64 = coarse.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.interpolate(c64.permute(0, 3, 1, 2), scale_factor=S, mode="bilinear").permute(0, 2, 3, 1)
    assert_close(fine, ref, dtype, "fine")
    g = torch.randn(B, h * S, w * S, C, device=dev()).to(dtype)
    gc = torch.full((B, h, w, C), float("nan"), device=dev(), dtype=dtype)
    _lib.check(L.mtlora_upsample_cl_bwd(_lib.ptr(g), _lib.ptr(gc), B, h, w, C, S, C, code, _lib.stream_ptr()), "bwd")
    ref.backward(g.double().cpu())
    assert_close(gc, c64.grad, dtype, "grad_coarse")


@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("B,Ltok,C", [(6, 49, 96), (3, 200, 384), (2, 50, 1536), (5, 7, 768)])
@pytest.mark.parametrize("rdt,ydt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32),
                                     (torch.float32, torch.float16)])
def test_residual_layer_norm_fused(rdt, ydt, B, Ltok, C, use_scale):
    """mtlora_residual_layernorm_fwd/bwd: x_new = shortcut + DropPath-scale * branch, y = LayerNorm(x_new); backward with
    gradients arriving on BOTH outputs (skip path + normalised path) against fp64 autograd of the composition, where the
    reference rounds x_new to the stream dtype before normalising (as the unfused kernels do)."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(B * C)
    sc_ = torch.randn(B, Ltok, C, device=dev()).to(rdt).requires_grad_(True)
    br = torch.randn(B, Ltok, C, device=dev()).to(ydt).requires_grad_(True)
    w = (1.0 + 0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    b = (0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    scale = ((torch.rand(B, device=dev()) < 0.7).float() / 0.7) if use_scale else None
    x_new, y = Fn.ResidualLayerNormFn.apply(sc_, br, scale, w, b, 1e-5, ydt)
    assert x_new.dtype == rdt and y.dtype == ydt
    g_skip, g_y = torch.randn_like(x_new), torch.randn_like(y)
    torch.autograd.backward([x_new, y], [g_skip, g_y])
    s64, b64, w64, bb64 = (t.detach().double().requires_grad_(True) for t in (sc_, br, w, b))
    sc64 = torch.ones(B, device=dev(), dtype=torch.float64) if scale is None else scale.double()
    xr = s64 + sc64.view(B, 1, 1) * b64
    xr_q = xr + (xr.detach().to(rdt).double() - xr.detach())  # straight-through rounding to the stream dtype
    yr = torch.nn.functional.layer_norm(xr_q, (C,), w64, bb64, 1e-5)
    torch.autograd.backward([xr_q, yr], [g_skip.double(), g_y.double()])
    assert_close(x_new, xr, rdt, "x_new")
    assert_close(y, yr, ydt, "y")
    assert_close(sc_.grad, s64.grad, rdt, "d_shortcut")
    assert_close(br.grad, b64.grad, ydt, "d_branch")
    assert_close(w.grad, w64.grad, ydt, "dgamma")
    assert_close(b.grad, bb64.grad, ydt, "dbeta")
    # only the skip path used: plain residual backward
    sc2, br2 = sc_.detach().clone().requires_grad_(True), br.detach().clone().requires_grad_(True)
    x2, _ = Fn.ResidualLayerNormFn.apply(sc2, br2, scale, w, b, 1e-5, ydt)
    x2.backward(g_skip)
    assert_close(sc2.grad, g_skip.double(), rdt, "d_shortcut (skip only)")
    assert_close(br2.grad, g_skip.double() * sc64.view(B, 1, 1), ydt, "d_branch (skip only)")


@pytest.mark.parametrize("xdt,autocast", [(torch.float32, True), (torch.bfloat16, True), (torch.float32, False)])
@pytest.mark.parametrize("n,B,H,W,C", [(5, 2, 8, 8, 96), (3, 2, 6, 10, 192), (2, 1, 4, 4, 384), (2, 1, 2, 2, 512)])
def test_layer_norm_merge_multi(xdt, autocast, n, B, H, W, C):
    """PatchMerging's norm over n token tensors in one launch (stacked output) == n single-tensor merge-gather LayerNorms:
    outputs bit-equal, input gradients bit-equal, dgamma / dbeta equal to the sum over the streams.  C = 512: 2048 normalised
    columns, the wide-row (8 vectors per lane) kernels in fp32 (8 vectors) and bf16 (4 vectors)."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(C + n)
    ln = torch.nn.LayerNorm(4 * C).to(dev())
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.1)
        ln.bias.normal_(0.0, 0.1)
    xs = [torch.randn(B, H * W, C, device=dev()).to(xdt).requires_grad_(True) for _ in range(n)]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ref = [Fn.layer_norm_merge(ln, x, H, W) for x in xs]
    g = [torch.randn_like(r) for r in ref]
    torch.autograd.backward(ref, g)
    gx_ref = [x.grad.clone() for x in xs]
    gw_ref, gb_ref = ln.weight.grad.clone(), ln.bias.grad.clone()
    for x in xs:
        x.grad = None
    ln.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        st = Fn.layer_norm_merge_multi(ln, xs, H, W)
    assert st is not None and st.shape == (n * B, H * W // 4, 4 * C) and st.dtype == ref[0].dtype
    for k in range(n):
        assert torch.equal(st[k * B:(k + 1) * B], ref[k])
    st.backward(torch.cat(g, 0))
    for k in range(n):
        assert torch.equal(xs[k].grad, gx_ref[k])
    dt = ref[0].dtype
    assert_close(ln.weight.grad, gw_ref.double(), dt, "dgamma")
    assert_close(ln.bias.grad, gb_ref.double(), dt, "dbeta")


@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("rdt,ydt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)])
@pytest.mark.parametrize("n,B,H,W,C", [(5, 2, 8, 8, 96), (3, 2, 6, 10, 192), (2, 3, 4, 4, 384), (2, 1, 2, 2, 512),
                                       (2, 1, 2, 4, 1024)])
def test_residual_merge_norm_streams(rdt, ydt, n, B, H, W, C, use_scale):
    """mtlora_residual_layernorm_streams_fwd/bwd with the PatchMerging gather (per-stream residual + DropPath folded into the
    merging LayerNorm, stacked output) == residual kernel + per-stream merge-gather LayerNorm: outputs and the residual /
    branch gradients bit-equal, dgamma / dbeta equal to the sum over the streams.  C = 512 / 1024: 2048 / 4096 normalised columns,
    the wide-row (8 vectors per lane) kernels; 4096 columns is the 16-bit limit and past the fp32 limit of 2048, where
    residual_merge_norm_streams answers None (its documented fallback: the caller forms the residuals itself)."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(3 * C + n)
    ln = torch.nn.LayerNorm(4 * C).to(dev())
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.1)
        ln.bias.normal_(0.0, 0.1)
    res = [torch.randn(B, H * W, C, device=dev()).to(rdt).requires_grad_(True) for _ in range(n)]
    brs = [torch.randn(B, H * W, C, device=dev()).to(ydt).requires_grad_(True) for _ in range(n)]
    if rdt == torch.float32 and 4 * C > 2048:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ydt == torch.bfloat16):
            assert Fn.residual_merge_norm_streams(ln, res, brs, H, W, 0.3 if use_scale else 0.0, True) is None
        return
    scale = ((torch.rand(n, B, device=dev()) < 0.7).float() / 0.7) if use_scale else None
    ac = ydt == torch.bfloat16
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
        xs = Fn.ResidualDropPathFn.apply(scale, False, n, *res, *brs)
        ref = [Fn.layer_norm_merge(ln, x, H, W) for x in xs]
    g = [torch.randn_like(r) for r in ref]
    torch.autograd.backward(ref, g)
    ref_g = [t.grad.clone() for t in res + brs]
    gw, gb = ln.weight.grad.clone(), ln.bias.grad.clone()
    for t in res + brs:
        t.grad = None
    ln.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
        st = Fn.ResidualMergeNormStreamsFn.apply(scale, ln.weight, ln.bias, ln.eps, ydt, H, W, n, *res, *brs)
    assert st.shape == (n * B, H * W // 4, 4 * C) and st.dtype == ydt
    for k in range(n):
        assert torch.equal(st[k * B:(k + 1) * B], ref[k]), k
    st.backward(torch.cat(g, 0))
    for t, r in zip(res, ref_g[:n]):
        assert torch.equal(t.grad, r)
    for k, (t, r) in enumerate(zip(brs, ref_g[n:])):
        if rdt == torch.float32 or scale is None:
            assert torch.equal(t.grad, r)
        else:  # bf16 stream: the unfused path scales the bf16-ROUNDED d_res, the fused kernel scales before rounding
            assert_close(t.grad, r.double(), ydt, f"d_branch{k}")
    assert_close(ln.weight.grad, gw.double(), ydt, "dgamma")
    assert_close(ln.bias.grad, gb.double(), ydt, "dbeta")


@pytest.mark.parametrize("use_scale", [True, False])
@pytest.mark.parametrize("n,B,Ltok,C", [(5, 4, 49, 96), (3, 2, 100, 384), (5, 2, 9, 768), (9, 2, 30, 192), (2, 2, 5, 1024)])
@pytest.mark.parametrize("rdt,ydt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)])
def test_residual_layer_norm_multi(rdt, ydt, n, B, Ltok, C, use_scale):
    """mtlora_residual_layernorm_multi_fwd/bwd (one shortcut, n branches, n normalised outputs; backward sums the shortcut
    gradient and the LayerNorm parameter gradients over the streams) against fp64 autograd of the per-stream composition;
    one y output and one skip output are left without a gradient (zero-materialised).  C = 1024 in fp32: 4 vectors per lane, the
    wide-row kernels."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(n * C)
    sc_ = torch.randn(B, Ltok, C, device=dev()).to(rdt).requires_grad_(True)
    brs = [torch.randn(B, Ltok, C, device=dev()).to(ydt).requires_grad_(True) for _ in range(n)]
    w = (1.0 + 0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    b = (0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    scale = ((torch.rand(n, B, device=dev()) < 0.7).float() / 0.7) if use_scale else None
    outs = Fn.ResidualLayerNormMultiFn.apply(scale, w, b, 1e-5, ydt, n, sc_, *brs)
    xs, ys = outs[:n], outs[n:]
    assert all(x.dtype == rdt for x in xs) and all(y.dtype == ydt for y in ys)
    g_skip = [torch.randn_like(x) for x in xs]
    g_y = [torch.randn_like(y) for y in ys]
    use_x = [k for k in range(n) if k != 1]      # stream 1: no skip gradient
    use_y = [k for k in range(n) if k != n - 1]  # last stream: normalised output unused
    torch.autograd.backward([xs[k] for k in use_x] + [ys[k] for k in use_y], [g_skip[k] for k in use_x] + [g_y[k] for k in use_y])
    s64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (sc_, w, b))
    br64 = [t.detach().double().requires_grad_(True) for t in brs]
    rx, ry = [], []
    for k in range(n):
        f = torch.ones(B, device=dev(), dtype=torch.float64) if scale is None else scale[k].double()
        xr = s64 + f.view(B, 1, 1) * br64[k]
        xq = xr + (xr.detach().to(rdt).double() - xr.detach())
        rx.append(xq)
        ry.append(torch.nn.functional.layer_norm(xq, (C,), w64, b64, 1e-5))
    torch.autograd.backward([rx[k] for k in use_x] + [ry[k] for k in use_y],
                            [g_skip[k].double() for k in use_x] + [g_y[k].double() for k in use_y])
    for k in range(n):
        assert_close(xs[k], rx[k], rdt, f"x_new{k}")
        assert_close(ys[k], ry[k], ydt, f"y{k}")
        # (n = 2: stream 1 is both the one without a skip gradient and the one without a y gradient -- autograd leaves its fp64
        # branch gradient unset, the kernel writes the zeros it stands for)
        assert_close(brs[k].grad, br64[k].grad if br64[k].grad is not None else torch.zeros_like(br64[k]), ydt, f"d_branch{k}")
    assert_close(sc_.grad, s64.grad, rdt, "d_shortcut")
    assert_close(w.grad, w64.grad, ydt, "dgamma")
    assert_close(b.grad, b64.grad, ydt, "dbeta")


@pytest.mark.parametrize("spread", [1.5, 5.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_tasks", [False, True])
def test_linear_bwd_gelu_fused(dtype, with_tasks, spread):
    """mtlora_linear_bwd_gelu: fc2(gelu(h)) with the GELU derivative applied inside fc2's dX kernel == the unfused
    composition (ATen gelu + gelu_backward), same dropout seeds; shared and per-task inputs, ragged M.  spread 5: pre-activations
    out to |h| ~ 20, past the |h| = 4.24 where the 16-bit kernels' polynomial erf saturates (common.h mtl_erf2n)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.lora import MTLoRALinear
    torch.manual_seed(3)
    tasks = ["a", "b"] if with_tasks else None
    r = {"shared": 16, "a": 4, "b": 4} if with_tasks else {"shared": 16}
    K, N, M = 192, 96, 777
    m = MTLoRALinear(K, N, r=r, lora_shared_scale=2.0, lora_task_scale={"a": 1.0, "b": 0.5} if with_tasks else 1.0,
                     lora_dropout=0.1, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if "lora_" in n_:
                p_.normal_(0, 0.1)
    m.train()
    hs = [(spread * torch.randn(3, M // 3, K, device=dev())).to(dtype).requires_grad_(True) for _ in range(1 + (2 if with_tasks else 0))]
    gys = None
    res = []
    for fused in (False, True):
        Fn._seed_counter = 1000
        for h in hs:
            h.grad = None
        m.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            if fused:
                a = [Fn.GeluDeferredGradFn.apply(h) for h in hs]
                y, yt = m(a[0], {t: a[1 + i] for i, t in enumerate(tasks)} if tasks else None,
                          gelu_gate=(hs[0], {t: hs[1 + i] for i, t in enumerate(tasks)} if tasks else None))
            else:
                a = [torch.nn.functional.gelu(h) for h in hs]
                y, yt = m(a[0], {t: a[1 + i] for i, t in enumerate(tasks)} if tasks else None)
        outs = [y] + ([yt[t] for t in tasks] if tasks else [])
        if gys is None:
            gys = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, gys)
        res.append(([o.detach().clone() for o in outs], [h.grad.clone() for h in hs],
                    {n_: p_.grad.clone() for n_, p_ in m.named_parameters() if p_.grad is not None}))
    (o0, g0, p0), (o1, g1, p1) = res
    for a_, b_ in zip(o0, o1):
        assert torch.equal(a_, b_)
    for i, (a_, b_) in enumerate(zip(g0, g1)):
        assert_close(b_, a_.double(), dtype, f"dh{i}")
    assert p0.keys() == p1.keys()
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


@pytest.mark.parametrize("spread", [1.0, 4.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_tasks", [False, True])
def test_mlp_gelu_fused_both_ways(dtype, with_tasks, spread):
    """fc1 -> GELU -> fc2 with the activation written by fc1's epilogue (mtlora_linear_fwd_gelu) and its derivative applied
    in fc2's dX epilogue (mtlora_linear_bwd_gelu) == the plain composition with ATen's gelu / gelu_backward: pre-activations
    bit-equal, activations / outputs / every gradient within tolerance (same dropout seeds)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.lora import MTLoRALinear
    torch.manual_seed(11)
    tasks = ["a", "b"] if with_tasks else None
    r = {"shared": 16, "a": 4, "b": 4} if with_tasks else {"shared": 16}
    sc = {"a": 1.0, "b": 0.5} if with_tasks else 1.0
    C, Hd, M = 96, 384, 3 * 211
    fc1 = MTLoRALinear(C, Hd, r=r, lora_shared_scale=2.0, lora_task_scale=sc, lora_dropout=0.1, tasks=tasks).to(dev())
    fc2 = MTLoRALinear(Hd, C, r=r, lora_shared_scale=2.0, lora_task_scale=sc, lora_dropout=0.1, tasks=tasks).to(dev())
    with torch.no_grad():
        for m_ in (fc1, fc2):
            for n_, p_ in m_.named_parameters():
                if "lora_" in n_:
                    p_.normal_(0, 0.1)
            m_.linear.weight.requires_grad_(False)
            m_.linear.bias.requires_grad_(False)
            m_.train()
    # (spread 4: pre-activations well past the saturation point of the 16-bit kernels' polynomial erf)
    xs = [(spread * torch.randn(3, M // 3, C, device=dev())).to(dtype).requires_grad_(True) for _ in range(1 + (2 if with_tasks else 0))]
    td = lambda lst: {t: lst[1 + i] for i, t in enumerate(tasks)} if tasks else None
    res, gys = [], None
    for fused in (False, True):
        Fn._seed_counter = 500
        for x in xs:
            x.grad = None
        fc1.zero_grad()
        fc2.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            if fused:
                h, h_t, a, a_t = fc1(xs[0], td(xs), gelu_out=True)
                y, y_t = fc2(a, a_t, gelu_gate=(h.detach(), None if h_t is None else {t: v.detach() for t, v in h_t.items()}))
            else:
                h, h_t = fc1(xs[0], td(xs))
                a = torch.nn.functional.gelu(h)
                a_t = {t: torch.nn.functional.gelu(h_t[t]) for t in tasks} if tasks else None
                y, y_t = fc2(a, a_t)
        outs = [y] + ([y_t[t] for t in tasks] if tasks else [])
        if gys is None:
            gys = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, gys)
        res.append((h.detach().clone(), a.detach().clone(), [o.detach().clone() for o in outs], [x.grad.clone() for x in xs],
                    {f"fc{i_}.{n_}": p_.grad.clone() for i_, m_ in enumerate((fc1, fc2), 1) for n_, p_ in m_.named_parameters()
                     if p_.grad is not None}))
    (h0, a0, o0, g0, p0), (h1, a1, o1, g1, p1) = res
    assert torch.equal(h0, h1)
    assert_close(a1, a0.double(), dtype, "gelu(h)")
    for i, (u, v) in enumerate(zip(o0, o1)):
        assert_close(v, u.double(), dtype, f"y{i}")
    for i, (u, v) in enumerate(zip(g0, g1)):
        assert_close(v, u.double(), dtype, f"dx{i}")
    assert p0.keys() == p1.keys() and len(p0) >= 4
    for k in p0:
        assert_close(p1[k], p0[k].double(), dtype, k)



def _mlp_with_tasks(tasks, C, Hd, r_s, r_t, p_drop, seed):
    from mtlora_amd.swin_transformer_mtlora import Mlp
    from mtlora_amd import mtl_harness as H
    torch.manual_seed(seed)
    ns = H.mtlora_namespace(tasks, r_shared=r_s, r_task=r_t, scale=2.0, dropout=p_drop)
    mlp = Mlp(C, Hd, lora=True, tasks=tasks, mtlora=ns, layer_idx=0).to(dev())
    with torch.no_grad():
        for n_, p_ in mlp.named_parameters():
            if "lora_" in n_:
                p_.normal_(0, 0.1)
            else:
                p_.requires_grad_(False)
    return mlp.train()


def _mlp_reference_fp64(mlp, xs, tasks, gys, q_floor=None, floors=None):
    """fc1 -> GELU -> fc2 of a task-enabled Mlp (reference lora.py:262-266 with x_tasks, swin_transformer_mtlora.py:68-81) in fp64,
    dropout off: outputs, input gradients and factor gradients"""
    P = {n: p.detach().double().requires_grad_(p.requires_grad) for n, p in mlp.named_parameters()}
    X = [x.detach().double().requires_grad_(True) for x in xs]

    def lin(pre, x, xt):
        W, b = P[f"{pre}.linear.weight"], P[f"{pre}.linear.bias"]
        base = x @ W.t() + b
        s = float(getattr(mlp, pre).lora_shared_scale)
        ys = base + s * (x @ P[f"{pre}.lora_shared_A"].t()) @ P[f"{pre}.lora_shared_B"].t()
        yt = []
        for i, t in enumerate(tasks):
            st = float(getattr(mlp, pre).lora_task_scale[t])
            yt.append(base + st * (xt[i] @ P[f"{pre}.lora_tasks_A.{t}"].t()) @ P[f"{pre}.lora_tasks_B.{t}"].t())
        return ys, yt
    h, ht = lin("fc1", X[0], X[1:])
    for v in ht:
        v.retain_grad()
    g = torch.nn.functional.gelu
    y, yt = lin("fc2", g(h), [g(v) for v in ht])
    outs = [y] + yt
    torch.autograd.backward(outs, [q.double() for q in gys])
    if q_floor is not None:
        # what ANY path that keeps Q1_t = s_t dH_t B1_t (M x r_t) in `q_floor` precision loses on dX_t = Q1_t A1_t: the exact Q rounded once
        for i, t in enumerate(tasks):
            st = float(mlp.fc1.lora_task_scale[t])
            Q = st * (ht[i].grad @ P[f"fc1.lora_tasks_B.{t}"].detach())
            dxq = Q.to(q_floor).double() @ P[f"fc1.lora_tasks_A.{t}"].detach()
            floors.append(((dxq - X[1 + i].grad).abs().max() / X[1 + i].grad.abs().max().clamp_min(1e-300)).item())
    return outs, [x.grad for x in X], {n: p.grad for n, p in P.items() if p.grad is not None}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("geom", ["c2s0", "t8", "r8", "wide", "t3mixed"])
def test_mlp_implicit_task_hiddens(dtype, geom):
    """``Fn.MlpHidFn`` (csrc/hid.hip: the task hidden tensors of a task-enabled Mlp never reach HBM) against (i) the per-layer path with the
    SAME dropout seeds -- train mode, p = 0.1 -- and (ii) the fp64 formulas of the reference (lora.py:262-266, Mlp :68-81), dropout off:
    outputs, every input gradient and every factor gradient at the north-star tolerance.  Geometries: Swin-T stage 0 of c2 (4 tasks of
    rank 4), 8 tasks (two task groups per launch), rank 8 (the rank-8 register geometry), hidden 2048 (1024-thread workgroups) and three
    tasks of mixed ranks with a row count that is no multiple of the row batch."""
    from mtlora_amd import functional as Fn
    C, Hd, T, r_t, M = {"c2s0": (96, 384, 4, 4, 3 * 977), "t8": (96, 384, 8, 4, 2 * 515), "r8": (192, 768, 2, 8, 1030),
                        "wide": (128, 2048, 4, 4, 2 * 301), "t3mixed": (96, 384, 3, 3, 1027)}[geom]
    tasks = [f"t{i}" for i in range(T)]
    tol = {torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype]
    for p_drop in (0.1, 0.0):
        mlp = _mlp_with_tasks(tasks, C, Hd, 16, r_t, p_drop, seed=23)
        xs = [torch.randn(M, C, device=dev()).requires_grad_(True) for _ in range(1 + T)]
        gys = None
        res = []
        for hid in (False, True):
            old = Fn.set_mlp_hid(hid)
            try:
                Fn._seed_counter = 900
                for x in xs:
                    x.grad = None
                mlp.zero_grad()
                with torch.autocast("cuda", dtype=dtype):
                    y, y_t = mlp(xs[0], {t: xs[1 + i] for i, t in enumerate(tasks)})
                outs = [y] + [y_t[t] for t in tasks]
                if gys is None:
                    gys = [torch.randn_like(o) for o in outs]
                torch.autograd.backward(outs, gys)
                res.append(([o.detach().clone() for o in outs], [x.grad.clone() for x in xs],
                            {n_: p_.grad.clone() for n_, p_ in mlp.named_parameters() if p_.grad is not None}))
            finally:
                Fn.set_mlp_hid(old)
        (o0, g0, p0), (o1, g1, p1) = res
        assert p0.keys() == p1.keys() and len(p0) == 4 * (1 + T)
        refs = [("per-layer path", o0, g0, p0, 1.0)]
        if p_drop == 0.0:
            ro, rg, rp = _mlp_reference_fp64(mlp, xs, tasks, gys)
            refs.append(("fp64 reference", ro, rg, rp, 1.0))
        for what, ro, rg, rp, mult in refs:
            for i, (u, v) in enumerate(zip(ro, o1)):
                e = rel_err(v, u)
                _log_parity(f"hid y{i} vs {what}", e, tol, mult)
                assert e <= tol * mult, (what, "y", i, e)
            for i, (u, v) in enumerate(zip(rg, g1)):
                e = rel_err(v, u)
                _log_parity(f"hid dx{i} vs {what}", e, tol, mult)
                assert e <= tol * mult, (what, "dx", i, e)
            for k in p1:
                e = rel_err(p1[k], rp[k])
                _log_parity(f"hid d{k} vs {what}", e, tol, mult)
                assert e <= tol * mult, (what, k, e)


@pytest.mark.parametrize("name", ["c2.s0", "c2.s1", "c2.s2", "c5r4.s0", "swinb.s1"])
def test_full_size_mlp_task_hiddens_vs_oracle(name):
    """the task-enabled Mlp of the benchmark configurations at FULL M (BASELINE configs[1] stages 0-2: 401 408 / 100 352 / 25 088 rows, hidden
    384 / 768 / 1536 = 1 / 2 / 4 column chunks; configs[4] with 8 tasks = two task groups; Swin-B's stage 1: hidden 1024 = 4 chunks of 256), bf16:
    ``Fn.MlpHidFn`` AND the per-layer path against the fp64 formulas of the reference (lora.py:262-266, Mlp :68-81; ATen fp64 on the GPU,
    dropout off -- train-mode masks are pinned by ``test_mlp_implicit_task_hiddens`` and ``FULL_T4``): every output, input gradient and factor
    gradient of the new path at the north-star tolerance; per ROW (a wrong row block or column chunk shows even when the global maximum hides
    it) the new path must stay within 3x the tolerance of the row's own scale, or within 1.5x of what the per-layer path loses on that tensor
    (the worst of 400 k rows is a cancellation row of a rank-4 product whose M x 4 factor Q is rounded to 16 bits on BOTH paths: 3.7 % vs
    4.1 % on the task input gradients of stage 0 -- two draws of the same rounding noise).  [auto]: the MFMA kernels the benchmark runs;
    [tiled]: the VALU forms."""
    from mtlora_amd import functional as Fn
    C, Hd, T, M = {"c2.s0": (96, 384, 4, 32 * 112 * 112), "c2.s1": (192, 768, 4, 32 * 56 * 56), "c2.s2": (384, 1536, 4, 32 * 28 * 28),
                   "c5r4.s0": (96, 384, 8, 32 * 112 * 112), "swinb.s1": (256, 1024, 4, 16 * 56 * 56)}[name]
    tasks = [f"t{i}" for i in range(T)]
    dtype, tol = torch.bfloat16, 1e-2
    mlp = _mlp_with_tasks(tasks, C, Hd, 64 if name != "c5r4.s0" else 4, 4, 0.0, seed=29)
    g = torch.Generator(device="cuda").manual_seed(5)
    xs = [torch.randn(M, C, device=dev(), generator=g).to(dtype).float().requires_grad_(True) for _ in range(1 + T)]
    gys = [torch.randn(M, C, device=dev(), generator=g).to(dtype) for _ in range(1 + T)]
    floors = []
    ro, rg, rp = _mlp_reference_fp64(mlp, xs, tasks, gys, q_floor=dtype, floors=floors)
    ro, rg = [t.detach() for t in ro], [t.detach() for t in rg]
    res = []
    for hid in (False, True):
        old = Fn.set_mlp_hid(hid)
        try:
            for x in xs:
                x.grad = None
            mlp.zero_grad()
            with torch.autocast("cuda", dtype=dtype):
                y, y_t = mlp(xs[0], {t: xs[1 + i] for i, t in enumerate(tasks)})
            outs = [y] + [y_t[t] for t in tasks]
            torch.autograd.backward(outs, gys)
            res.append(([o.detach().double() for o in outs], [x.grad.double() for x in xs],
                        {n_: p_.grad.clone() for n_, p_ in mlp.named_parameters() if p_.grad is not None}))
            del outs, y, y_t
        finally:
            Fn.set_mlp_hid(old)
    (o0, g0, p0), (o1, g1, p1) = res
    assert p0.keys() == p1.keys() and len(p0) == 4 * (1 + T)

    def row_err(v, u):  # against the row's own scale, floored at a tenth of the tensor's (rows of tiny norm carry rounding only)
        rs = u.abs().amax(dim=1).clamp_min(0.1 * u.abs().max().clamp_min(1e-12))
        return ((v - u).abs().amax(dim=1) / rs).max().item()
    for what, ref, per_layer, got in (("y", ro, o0, o1), ("dx", rg, g0, g1)):
        for i, (u, w, v) in enumerate(zip(ref, per_layer, got)):
            e = ((v - u).abs().max() / u.abs().max().clamp_min(1e-12)).item()
            e_old = ((w - u).abs().max() / u.abs().max().clamp_min(1e-12)).item()
            # the north-star tolerance; for the task input gradients dX_t = Q1_t A1_t -- a rank-4 product whose M x 4 factor BOTH paths (and the
            # reference under autocast) keep in 16 bits -- plus what the exact Q rounded once to 16 bits loses on that tensor (measured above:
            # 0.24-0.31 %; the per-layer path reads 0.65-1.03 % on the same tensors, this one 0.70-1.12 %)
            fl = floors[i - 1] if (what == "dx" and i >= 1) else 0.0
            _log_parity(f"full-size hid {what}{i} {name} (per-layer path: {e_old:.3e}, 16-bit Q floor: {fl:.3e})", e, tol, 1.0)
            assert e <= tol + fl, (name, what, i, e, e_old, fl)
            er, er_old = row_err(v, u), row_err(w, u)
            _log_parity(f"full-size hid {what}{i} per row {name} (per-layer path: {er_old:.3e})", er, tol, 3.0)
            assert er <= max(3.0 * tol, 1.5 * er_old), (name, what, i, "row", er, er_old)
    for k in p1:
        e = rel_err(p1[k], rp[k])
        _log_parity(f"full-size hid d{k} {name}", e, tol, 1.0)
        assert e <= tol, (name, k, e)


# ------------------------------------------------------------------------------------------------
# fused bilinear upsample + loss (+ backward)
# ------------------------------------------------------------------------------------------------
def _loss_case(task, B, h, w, S, seed):
    g = torch.Generator().manual_seed(seed)
    C = O.NUM_OUTPUT[task]
    low = torch.randn(B, h, w, C, generator=g) * 2.0
    H, W = h * S, w * S
    if task in ("semseg", "human_parts"):
        lab = torch.randint(0, C, (B, 1, H, W), generator=g).float()
        lab[torch.rand(B, 1, H, W, generator=g) < 0.07] = 255.0
    elif task == "normals":
        lab = torch.nn.functional.normalize(torch.randn(B, 3, H, W, generator=g), dim=1)
        lab[torch.rand(B, 3, H, W, generator=g) < 0.05] = 255.0
    else:
        lab = (torch.rand(B, 1, H, W, generator=g) < 0.3).float()
    return low, lab


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("task,B,h,w,S", [("semseg", 2, 20, 20, 4), ("human_parts", 3, 18, 33, 4), ("normals", 2, 37, 16, 4),
                                          ("sal", 2, 16, 16, 4), ("semseg", 1, 7, 9, 2), ("sal", 2, 5, 40, 3),
                                          ("normals", 1, 16, 16, 1),
                                          # the scale the models actually run at (stage-1 maps 56 -> 448 / 28 -> 224: S = 8)
                                          ("normals", 2, 28, 28, 8), ("semseg", 2, 28, 28, 8), ("sal", 1, 28, 28, 8),
                                          ("human_parts", 1, 14, 21, 8),
                                          # tile geometry of the wave-per-tile kernel: TQ = 64 / S - 1 columns (63 at S = 1, 3 at
                                          # S = 16, 1 at S = 32), several column tiles, a last partial row tile, batch offsets
                                          ("normals", 3, 9, 70, 1), ("sal", 2, 6, 5, 16), ("semseg", 1, 5, 4, 32),
                                          ("human_parts", 5, 13, 15, 8), ("semseg", 2, 9, 23, 3)])
def test_upsample_loss_vs_oracle(task, B, h, w, S, dtype):
    """value and gradient of loss(interpolate(low)) against the oracle's task_loss on torch's own bilinear upsample
    (fp64 on the CPU), incl. partial tiles, h != w, borders, ignore_index pixels and scales 1..32."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.mtl_harness import MultiTaskLoss
    low, lab = _loss_case(task, B, h, w, S, seed=h * 100 + w)
    low_q = low.to(dtype)
    ref_in = low_q.double().requires_grad_(True)
    up = torch.nn.functional.interpolate(ref_in.permute(0, 3, 1, 2), scale_factor=S, mode="bilinear")
    ref = O.task_loss(task, up, lab.double())
    ref.backward()
    x = low_q.to(dev()).requires_grad_(True)
    got = Fn.UpsampleLossFn.apply(MultiTaskLoss.FUSED_KIND[task], x, lab.to(dev()), S)
    (got * 3.0).backward()
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    assert abs(got.item() - ref.item()) <= tol * max(1.0, abs(ref.item())), (got.item(), ref.item())
    e = rel_err(x.grad.float() / 3.0, ref_in.grad)
    assert e <= (1e-4 if dtype == torch.float32 else 1e-2), e


def test_fused_loss_path_equals_plain_path():
    """MultiTaskLoss.forward_low(low) == MultiTaskLoss.forward(F.interpolate(low)) (value and gradient) on the GPU."""
    from mtlora_amd.mtl_harness import MultiTaskLoss
    tasks = ["semseg", "normals", "sal", "human_parts"]
    crit = MultiTaskLoss(tasks)
    low, gt = {}, {}
    for i, t in enumerate(tasks):
        lo, lab = _loss_case(t, 2, 24, 24, 4, seed=i)
        low[t], gt[t] = lo.to(dev()).requires_grad_(True), lab.to(dev())
    total, per = crit.forward_low(low, gt)
    total.backward()
    g_fused = {t: low[t].grad.clone() for t in tasks}
    for t in tasks:
        low[t].grad = None
    pred = {t: torch.nn.functional.interpolate(low[t].permute(0, 3, 1, 2), scale_factor=4, mode="bilinear") for t in tasks}
    total2, per2 = crit(pred, gt)
    total2.backward()
    assert abs(total.item() - total2.item()) <= 1e-4 * abs(total2.item())
    for t in tasks:
        assert abs(per[t].item() - per2[t].item()) <= 1e-4 * max(1.0, abs(per2[t].item())), t
        assert rel_err(g_fused[t], low[t].grad) <= 1e-4, t


def test_fused_loss_at_the_heads_size():
    """the four fused upsample + loss kernels at the geometry the c2 heads run at (56 x 56 -> 448 x 448, S = 8; B = 8, bf16 logits)
    against ATen's interpolate + the plain losses on the same GPU in fp32: value and gradient.  (Label tensors are sized exactly:
    a read past the last batch entry's channels faults here, not in the small oracle cases.)"""
    from mtlora_amd.mtl_harness import MultiTaskLoss
    tasks = ["semseg", "normals", "sal", "human_parts"]
    crit = MultiTaskLoss(tasks)
    low, gt = {}, {}
    for i, t in enumerate(tasks):
        lo, lab = _loss_case(t, 8, 56, 56, 8, seed=40 + i)
        low[t], gt[t] = lo.to(dev()).bfloat16().requires_grad_(True), lab.to(dev()).clone()
    total, per = crit.forward_low(low, gt)
    total.backward()
    g_fused = {t: low[t].grad.float().clone() for t in tasks}
    ref_in = {t: low[t].detach().float().requires_grad_(True) for t in tasks}
    pred = {t: torch.nn.functional.interpolate(ref_in[t].permute(0, 3, 1, 2), scale_factor=8, mode="bilinear") for t in tasks}
    total2, per2 = crit(pred, gt)
    total2.backward()
    for t in tasks:
        assert abs(per[t].item() - per2[t].item()) <= 1e-3 * max(1.0, abs(per2[t].item())), (t, per[t].item(), per2[t].item())
        e = rel_err(g_fused[t], ref_in[t].grad)
        _log_parity(f"fused loss at 56x56 x8 d_low {t}", e, 1e-2, 1.0)
        assert e <= 1e-2, (t, e)  # (the fused gradient is rounded to bf16 once)


# ------------------------------------------------------------------------------------------------
# device-side seed offset (ABI v2) and the HIP-graph train step
# ------------------------------------------------------------------------------------------------
def test_linear_seed_offset_is_added_on_device():
    """mtlora_linear_desc.seed_offset: the kernels use seed + *offset (mod 2^64), forward and backward."""
    from mtlora_amd.lora import MTLoRALinear
    from mtlora_amd import functional as Fn
    M, K, N = 257, 96, 128
    torch.manual_seed(5)
    m = MTLoRALinear(K, N, r={"shared": 16}, lora_shared_scale=2.0, lora_task_scale=1.0, lora_dropout=0.25, tasks=None).to(dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * 0.05)
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    x = torch.randn(M, K, device=dev(), requires_grad=True)
    off = torch.tensor([0x1E3779B97F4A7C15 * 3 % (1 << 63)], dtype=torch.int64, device=dev())
    try:
        Fn.set_seed_offset(off)
        c0 = Fn._seed_counter
        y, _ = m(x, None)
        Fn._seed_counter = c0
        seed = (Fn.next_seed() + int(off.item())) & 0xFFFFFFFFFFFFFFFF
        keep = O.dropout_keep_mask(seed, 0, M, K, 0.25)
        P, xs, _, yo, _ = _oracle_linear(m, x, None, keep=keep, p=0.25)
        assert_close(y, yo, torch.float32, "y")
        y.sum().backward()
        yo.sum().backward()
        assert_close(x.grad, xs.grad, torch.float32, "dx")
        for n, p in m.named_parameters():
            if p.requires_grad:
                assert_close(p.grad, P[n].grad, torch.float32, f"grad {n}")
        # a different offset -> a different mask
        off.add_(12345)
        y2, _ = m(x, None)   # NB: draws the next host seed as well; only checks that the result moved
        assert not torch.allclose(y2, y)
    finally:
        Fn.set_seed_offset(None)


def test_library_is_hip_graph_safe():
    """The library's launches can be captured into a HIP graph and replayed: MTLoRALinear forward + backward with an
    UNUSED task output (the backward must zero that output's slice of Q) inside torch.cuda.graph, with the graph's
    private pool dirtied between uses.  Guards the zero-fill-as-a-kernel rule (common.h:mtl_zero_async): a captured
    small hipMemsetAsync does not take effect from the second replay on with this ROCm stack (stale pool memory shows
    through), which is also why bench.py does not replay the whole train step as a graph by default."""
    from mtlora_amd.lora import MTLoRALinear
    M, K, N = 640, 96, 192
    tasks = ["a", "b"]
    torch.manual_seed(11)
    m = MTLoRALinear(K, N, r={"shared": 16, "a": 4, "b": 4}, lora_shared_scale=2.0, lora_task_scale={"a": 1.0, "b": 1.0},
                     lora_dropout=0.0, tasks=tasks).to(dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * 0.05)
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    x = torch.randn(M, K, device=dev(), dtype=torch.bfloat16, requires_grad=True)
    xt = {t: torch.randn(M, K, device=dev(), dtype=torch.bfloat16, requires_grad=True) for t in tasks}
    gy = torch.randn(M, N, device=dev(), dtype=torch.bfloat16)

    def run():
        junk = torch.full((1 << 16,), float("nan"), device=dev())  # dirty a pool block the scratch buffers may reuse
        del junk
        y, yt = m(x, xt)
        (y * gy).sum().backward(inputs=[x, xt["a"], xt["b"]] + [p for p in m.parameters() if p.requires_grad])
        # yt["a"], yt["b"] unused: their gradients are undefined -> zero-filled slices inside the library

    grads = lambda: [x.grad, xt["a"].grad, xt["b"].grad] + [p.grad for p in m.parameters() if p.requires_grad]  # noqa: E731

    def clear():
        x.grad = None
        for t in tasks:
            xt[t].grad = None
        for p in m.parameters():
            p.grad = None

    run()
    ref = [None if g is None else g.clone() for g in grads()]
    clear()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    clear()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(4):
        g.replay()
        torch.cuda.synchronize()
        for a_, b_ in zip(grads(), ref):
            assert (a_ is None) == (b_ is None)
            if a_ is not None:
                assert torch.isfinite(a_).all()
                assert torch.equal(a_, b_)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_concat_upsample_vs_torch(dtype):
    """ConcatUpsampleFn == torch.cat([x0, F.interpolate(x1), F.interpolate(x2), ...], channels) on the padded layout,
    values and gradients (scales 2 / 4 / 8, H != W)."""
    from mtlora_amd import functional as Fn
    B, H, W = 2, 16, 24
    chans = [18, 36, 72, 144]
    torch.manual_seed(0)
    maps = [torch.randn(B, H >> i, W >> i, c, device=dev()).to(dtype).requires_grad_(True) for i, c in enumerate(chans)]
    out = Fn.ConcatUpsampleFn.apply(*maps)
    offs, ld = Fn.ConcatUpsampleFn.layout(chans)
    assert out.shape == (B * H * W, ld) and ld % 8 == 0
    refs = [m.detach().double().requires_grad_(True) for m in maps]
    ups = [refs[0]] + [torch.nn.functional.interpolate(r.permute(0, 3, 1, 2), (H, W), mode="bilinear").permute(0, 2, 3, 1)
                       for r in refs[1:]]
    o3 = out.view(B, H, W, ld)
    used = torch.zeros(ld, dtype=torch.bool)
    for o, c, u in zip(offs, chans, ups):
        assert_close(o3[..., o:o + c], u, dtype, f"slice@{o}")
        used[o:o + c] = True
    assert (o3[..., ~used.to(o3.device)] == 0).all()   # pad channels are zero
    g = torch.randn(B * H * W, ld, device=dev()).to(dtype)
    out.backward(g)
    g3 = g.view(B, H, W, ld).double().cpu()
    sum((u.cpu() * g3[..., o:o + c]).sum() for o, c, u in zip(offs, chans, ups)).backward()
    for m, r in zip(maps, refs):
        assert_close(m.grad, r.grad, dtype, "grad")


# ------------------------------------------------------------------------------------------------
# BASELINE configs[1] FULL sizes (B = 32, 448 x 448 -> M = 32 * 112 * 112 rows at stage 0): size-independent properties
# ------------------------------------------------------------------------------------------------
def test_full_size_linear_rows_vs_oracle():
    """MTLoRALinear at the full stage-0 size (M = 401 408, K = 96, N = 384, 4 tasks reading their own x_t, bf16):
    rows are independent, so (a) 2 048 sampled rows must match the oracle evaluated on those rows alone, forward and
    dX, and (b) the eval-mode map minus its bias is linear: f(x1 + x2) = f(x1) + f(x2)."""
    from mtlora_amd.lora import MTLoRALinear
    M, K, N = 32 * 112 * 112, 96, 384
    tasks = ["semseg", "normals", "sal", "human_parts"]
    dtype = torch.bfloat16
    torch.manual_seed(1)
    m = MTLoRALinear(K, N, r={"shared": 64, **{t: 4 for t in tasks}}, lora_shared_scale=4.0,
                     lora_task_scale={t: 4.0 for t in tasks}, lora_dropout=0.0, tasks=tasks).to(dev())
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn_like(p) * (0.05 if "lora" in n else 0.02)).to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    x = (torch.randn(M, K, device=dev()) * 0.5).to(dtype).requires_grad_(True)
    xt = {t: (torch.randn(M, K, device=dev()) * 0.5).to(dtype).requires_grad_(True) for t in tasks}
    y, yt = m(x, xt)
    idx = torch.randperm(M, device=dev())[:2048].sort().values
    gy = torch.zeros(M, N, device=dev(), dtype=dtype)
    gy[idx] = torch.randn(2048, N, device=dev()).to(dtype)
    gt = {t: torch.zeros(M, N, device=dev(), dtype=dtype) for t in tasks}
    for t in tasks:
        gt[t][idx] = torch.randn(2048, N, device=dev()).to(dtype)
    loss = (y.float() * gy.float()).sum() + sum((yt[t].float() * gt[t].float()).sum() for t in tasks)
    loss.backward(inputs=[x] + [xt[t] for t in tasks])
    # oracle on the sampled rows only
    xs = x.detach()[idx].clone().requires_grad_(True)
    xts = {t: xt[t].detach()[idx].clone().requires_grad_(True) for t in tasks}
    P, xo, xto, yo, yto = _oracle_linear(m, xs, xts)
    assert_close(y[idx], yo, dtype, "y rows")
    lo = (yo * gy[idx].double().cpu()).sum()
    for t in tasks:
        assert_close(yt[t][idx], yto[t], dtype, f"y[{t}] rows")
        lo = lo + (yto[t] * gt[t][idx].double().cpu()).sum()
    lo.backward()
    assert_close(x.grad[idx], xo.grad, dtype, "dx rows")
    for t in tasks:
        assert_close(xt[t].grad[idx], xto[t].grad, dtype, f"dx[{t}] rows")
    keep = torch.ones(M, dtype=torch.bool, device=dev())
    keep[idx] = False
    assert x.grad[keep].abs().max().item() == 0.0   # rows without an output gradient get an exactly zero dX
    # linearity in eval mode (bias removed), full size
    m.eval()
    with torch.no_grad():
        x1, x2 = x.detach()[: M // 2], x.detach()[M // 2:]
        f = lambda v: m(v, None)[0].float() - m.linear.bias.float()  # noqa: E731
        lhs, rhs = f((x1.float() + x2.float()).to(dtype)), f(x1) + f(x2)
        assert ((lhs - rhs).abs().max() / rhs.abs().max()).item() < 2e-2


def test_linear_accepts_strided_and_wider_inputs():
    """MTLoRALinear takes what nn.Linear takes: a NON-contiguous input (a transposed view), a 4-D input, an fp32 input under bf16
    autocast (cast inside) and a 1-D input; outputs keep the leading shape, gradients come back in the input's dtype and shape
    (the Function passes tensors to the kernels as they come and only copies what is not contiguous in the compute dtype)."""
    from mtlora_amd.lora import MTLoRALinear
    torch.manual_seed(5)
    tasks = ["a", "b"]
    m = MTLoRALinear(64, 96, r={"shared": 16, "a": 8, "b": 8}, lora_shared_scale=2.0, lora_task_scale={"a": 1.5, "b": 0.5}, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_(torch.randn_like(q) * (0.1 if "lora" in n_ else 0.05))
    m.eval()
    P = {k: v.detach().double() for k, v in m.named_parameters()}

    def ref(x64):
        y, yt = O.mtlora_linear(x64, P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                                tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                                scale_t=m.lora_task_scale)
        return y, yt

    base = torch.randn(3, 64, 10, device=dev())                       # (B, K, L)
    for name, x in (("transposed view", base.transpose(1, 2)),         # (B, L, K), stride (640, 1, 10)
                    ("4-D", torch.randn(2, 3, 5, 64, device=dev())),
                    ("1-D", torch.randn(64, device=dev()))):
        x = x.detach().requires_grad_(True)
        y, yt = m(x)
        assert y.shape == (*x.shape[:-1], 96) and all(yt[t].shape == y.shape for t in tasks), name
        (y.sum() + 2.0 * yt["a"].sum() - yt["b"].sum()).backward()
        xo = x.detach().double().requires_grad_(True)
        yo, yto = ref(xo)
        (yo.sum() + 2.0 * yto["a"].sum() - yto["b"].sum()).backward()
        assert_close(y, yo.detach(), torch.float32, f"{name} y")
        assert_close(yt["b"], yto["b"].detach(), torch.float32, f"{name} y_b")
        assert x.grad.shape == x.shape and x.grad.dtype == x.dtype, name
        assert_close(x.grad, xo.grad, torch.float32, f"{name} dx")
    x = torch.randn(4, 7, 64, device=dev(), requires_grad=True)       # fp32 in, bf16 compute
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, yt = m(x)
    assert y.dtype == torch.bfloat16 and y.shape == (4, 7, 96)
    y.float().sum().backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    yo, _ = ref(x.detach().double())
    assert_close(y, yo, torch.bfloat16, "autocast y")


@pytest.mark.parametrize("geom", [
    # (M, K, N, rank, dtype, p): k_pq forced (sel_projk = 3) on shapes off its tile grid
    (1000, 40, 72, 8, torch.bfloat16, 0.25),      # ragged last k-tile (K = 40: one full + one quarter), R = 8 (16-column stride), ragged M
    (777, 104, 200, 24, torch.bfloat16, 0.25),    # K = 3.25 k-tiles, R = 24 -> R stride 32: the 64-column tile is half empty
    (4097, 200, 104, 72, torch.float16, 0.1),     # R = 72 -> 128-column tile 62 % full, one row past a tile boundary, fp16
    (130, 520, 136, 128, torch.bfloat16, 0.0),    # unmasked (column-split wave grid), K = 16.25 k-tiles (> ring depth), R = 128
    (130, 520, 136, 128, torch.bfloat16, 0.5),    # the same masked (k-split wave grid)
    (24000, 96, 96, 64, torch.bfloat16, 0.05),    # > 1.25 residency rounds of 64-row tiles: the 128-row form (4 x 1 wave grid)
    (700, 384, 200, 256, torch.bfloat16, 0.1),    # rank stride 256: two 128-column tiles (blockIdx.y)
    (300, 136, 72, 328, torch.float16, 0.0),      # rank stride 336: three column tiles, the last one 62 % full
])
def test_pq_kernel_off_grid_shapes(geom, lowrank_form):
    """k_pq (csrc/pq.h) on shapes that do not line up with its tiles: ragged M, K not a multiple of the 32-wide k-tile (zero-page
    chunks), rank strides of 16 - 128 (half-empty column tiles, clamped projection rows), more k-tiles than ring stages, both wave grids
    and both tile heights -- forward, dX and both factor gradients against the fp64 oracle with the specified dropout mask."""
    from mtlora_amd import functional as Fn
    M, K, N, r, dtype, p = geom
    torch.manual_seed(M + K)
    m = _t0_layer(K, N, r, dtype, p, scale=2.0)
    prev = Fn.set_tuning(projk=3)
    try:
        got, ref, keep = _t0_train_case(m, M, dtype, p, None, torch.device("cpu") if M < 5000 else dev())
    finally:
        Fn.set_tuning(**prev)
    assert_close(got["y"], ref["y"], dtype, "y")
    assert_close(got["dx"], ref["dx"], dtype, "dx")
    assert_close(got["dA"], ref["dA"], dtype, "dA")
    assert_close(got["dB"], ref["dB"], dtype, "dB")


_M0, _M1, _M2 = 32 * 112 * 112, 32 * 56 * 56, 32 * 28 * 28
FULL_T0 = {  # BASELINE configs[1] layers without tasks, full M: name -> (M, K, N, kind)
    "s0.qkv": (_M0, 96, 288, None), "s0.proj": (_M0, 96, 96, None), "s0.fc1": (_M0, 96, 384, "gelu_out"),
    "s0.fc2": (_M0, 384, 96, "gate"), "s1.qkv": (_M1, 192, 576, None), "s1.fc1": (_M1, 192, 768, "gelu_out"),
    "s1.fc2": (_M1, 768, 192, "gate"), "s2.qkv": (_M2, 384, 1152, None), "s2.fc1": (_M2, 384, 1536, "gelu_out"),
    "s2.fc2": (_M2, 1536, 384, "gate"), "s3.qkv": (32 * 14 * 14, 768, 2304, None), "s3.fc2": (32 * 14 * 14, 3072, 768, "gate"),
    # BASELINE configs[3] (Swin-B / 448, B = 16, rank 128), stage 2 -- the shapes k_pq exists for (64-row tiles, masked P with the
    # k-split wave grid, unmasked Q with the column-split one), and stage 1 (128-row tiles)
    "b2.qkv": (16 * 28 * 28, 512, 1536, None, 128), "b2.proj": (16 * 28 * 28, 512, 512, None, 128),
    "b2.fc1": (16 * 28 * 28, 512, 2048, "gelu_out", 128), "b2.fc2": (16 * 28 * 28, 2048, 512, "gate", 128),
    "b1.fc2": (16 * 56 * 56, 1024, 256, "gate", 128),
}


@pytest.mark.parametrize("name", list(FULL_T0))
def test_full_size_linear_t0_train_vs_oracle(name):
    """the T = 0 layers of BASELINE configs[1] at FULL size (B = 32: M = 401 408 / 100 352 / 25 088 rows), bf16, TRAIN mode with
    the reference's p = 0.05 and the mask of oracle.dropout_keep_mask: every output row, every dX row and the factor gradients
    reduced over the FULL M against the fp64 oracle (ATen fp64 on the GPU).  This is the only place where the persistent kernels
    run in the regime the benchmark times: a wave of k_sp_xres / k_sp_ares / k_sp_tn owns 6 - 49 slabs, a k_ntd workgroup walks
    several tiles with its ring running across them, k_ntl takes its 192-wide tile."""
    M, K, N, kind, *rank = FULL_T0[name]
    dtype, p = torch.bfloat16, 0.05
    torch.manual_seed(len(name) + K + N)
    m = _t0_layer(K, N, rank[0] if rank else 64, dtype, p, scale=4.0)
    got, ref, keep = _t0_train_case(m, M, dtype, p, kind, dev(), in_scale=0.5)
    assert abs(keep.float().mean().item() - 0.95) < 0.002
    assert_close(got["y"], ref["y"], dtype, f"{name} y")
    if kind == "gelu_out":
        assert_close(got["a"], ref["a"], dtype, f"{name} gelu(y)")
    assert_close(got["dx"], ref["dx"], dtype, f"{name} dx")
    assert_close(got["dA"], ref["dA"], dtype, f"{name} dA")
    assert_close(got["dB"], ref["dB"], dtype, f"{name} dB")
    # per-row check as well: max |err| relative to the ROW's own scale must not blow up anywhere (a wrong slab / tile shows here
    # even when the global maximum hides it)
    e = (got["y"].double() - ref["y"]).abs().amax(1) / ref["y"].abs().amax(1).clamp_min(1e-6)
    assert e.max().item() < 0.05, f"{name}: worst row of y off by {e.max().item():.3e} (row {int(e.argmax())})"
    e = (got["dx"].double() - ref["dx"]).abs().amax(1) / ref["dx"].abs().amax(1).clamp_min(ref["dx"].abs().max().item() * 1e-2)
    assert e.max().item() < 0.1, f"{name}: worst row of dx off by {e.max().item():.3e} (row {int(e.argmax())})"


_MB1, _MB2 = 16 * 56 * 56, 16 * 28 * 28
FULL_T4 = {  # the task-enabled layers (last block of a stage), full M: name -> (M, K, N, x_tasks, gate[, n_tasks, r_shared, r_task])
    # BASELINE configs[1]: 4 tasks of rank 4 next to the shared rank 64
    "s0.projT": (_M0, 96, 96, False, False), "s0.fc1T": (_M0, 96, 384, True, False), "s0.fc2T": (_M0, 384, 96, True, True),
    "s1.fc1T": (_M1, 192, 768, True, False), "s1.fc2T": (_M1, 768, 192, True, True), "s2.fc2T": (_M2, 1536, 384, True, True),
    # BASELINE configs[3] (Swin-B / 448, B = 16): 4 tasks, rank 128 shared AND per task -> R = 640, the multi-source k_pq passes (one
    # grid slice per source), with and without the tasks' own inputs, with the GELU' gates
    "b1.projT": (_MB1, 256, 256, False, False, 4, 128, 128), "b1.fc1T": (_MB1, 256, 1024, True, False, 4, 128, 128),
    "b1.fc2T": (_MB1, 1024, 256, True, True, 4, 128, 128), "b2.fc2T": (_MB2, 2048, 512, True, True, 4, 128, 128),
    # BASELINE configs[4]: 8 tasks at the two ends of the rank sweep
    "c5r4.s0.fc1T": (_M0, 96, 384, True, False, 8, 4, 4), "c5r4.s0.fc2T": (_M0, 384, 96, True, True, 8, 4, 4),
    "c5r256.s1.fc1T": (_M1, 192, 768, True, False, 8, 256, 256), "c5r256.s1.fc2T": (_M1, 768, 192, True, True, 8, 256, 256),
}
_TASKS8 = ["semseg", "normals", "sal", "human_parts", "t4", "t5", "t6", "t7"]


@pytest.mark.parametrize("name", list(FULL_T4))
def test_full_size_linear_t4_train_vs_oracle(name):
    """the layers WITH task outputs at full size, bf16, TRAIN mode (p = 0.05, specified mask): 4 tasks of rank 4 next to the shared rank
    64 (c2), 4 tasks of rank 128 next to a shared rank 128 (c4), 8 tasks of rank 4 / 256 (c5), with and without their own task
    inputs, fc2 with the GELU' gates -- all 1 + T outputs, dX, every dX_t and all 2 + 2 T factor gradients reduced over the full M
    against the fp64 oracle on the GPU (k_sp_proj / k_sp_projsum / k_pq multi-source / k_rank_out / the multi-output tile kernels /
    k_sp_tn in the regime the benchmark times)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.lora import MTLoRALinear
    M, K, N, use_xt, gate, *more = FULL_T4[name]
    nt, r_s, r_t = more if more else (4, 64, 4)
    tasks = _TASKS8[:nt]
    dtype, p = torch.bfloat16, 0.05
    torch.manual_seed(len(name) + K)
    m = MTLoRALinear(K, N, r={"shared": r_s, **{t: r_t for t in tasks}}, lora_shared_scale=4.0, lora_task_scale={t: 4.0 for t in tasks},
                     lora_dropout=p, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_((torch.randn_like(q) * (0.05 if "lora" in n_ else 0.02)).to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    n_in = 1 + (len(tasks) if use_xt else 0)
    c0 = Fn._seed_counter
    if gate:  # inputs are gelu(h): the dX kernels multiply by gelu'(h)
        hs = [(0.75 * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True) for _ in range(n_in)]
        xs_in = [Fn.GeluDeferredGradFn.apply(h) for h in hs]
        y, yt = m(xs_in[0], {t: xs_in[1 + i] for i, t in enumerate(tasks)} if use_xt else None,
                  gelu_gate=(hs[0], {t: hs[1 + i] for i, t in enumerate(tasks)} if use_xt else None))
        leaves = hs
    else:
        xs_in = [(0.5 * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True) for _ in range(n_in)]
        y, yt = m(xs_in[0], {t: xs_in[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
        leaves = xs_in
    Fn._seed_counter = c0
    seed = Fn.next_seed()
    outs = [y] + [yt[t] for t in tasks]
    gys = [torch.randn(M, N, device=dev()).to(dtype) for _ in outs]
    torch.autograd.backward(outs, gys)
    # ---- oracle in fp64 on the GPU
    keep = O.dropout_keep_mask_t(seed, 0, M, K, p, device=dev())
    P = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xo = [x.detach().double().requires_grad_(True) for x in xs_in]
    yo, yto = O.mtlora_linear(xo[0], P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                              tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                              scale_t=m.lora_task_scale, x_tasks={t: xo[1 + i] for i, t in enumerate(tasks)} if use_xt else None,
                              keep_mask=keep, p=p)
    outs_o = [yo] + [yto[t] for t in tasks]
    torch.autograd.backward(outs_o, [g.double() for g in gys])
    for i, (a, b) in enumerate(zip(outs, outs_o)):
        assert_close(a, b.detach(), dtype, f"{name} y[{i}]")
    for i, leaf in enumerate(leaves):
        ref = xo[i].grad
        if gate:
            hd = leaf.detach().double().requires_grad_(True)
            torch.nn.functional.gelu(hd).backward(ref)
            ref = hd.grad
        assert_close(leaf.grad, ref, dtype, f"{name} dx[{i}]")
    for n_, q in m.named_parameters():
        if q.requires_grad:
            assert_close(q.grad, P[n_].grad, dtype, f"{name} grad {n_}")


@pytest.mark.parametrize("geom", [
    # (M, K, N, n_tasks, r_shared, r_task, x_tasks, dtype, p): MULTI-SOURCE k_pq (one grid slice per source) forced on off-grid shapes
    (1000, 72, 104, 4, 24, 24, True, torch.bfloat16, 0.25),    # ragged M and K, rank stride 32 per source, masked shared source only
    (4097, 136, 72, 4, 128, 128, True, torch.bfloat16, 0.1),   # c4's geometry in small: R = 640, five sources, one row past a tile
    (4097, 136, 72, 4, 128, 128, False, torch.bfloat16, 0.1),  # the tasks read D(X): ONE masked source, five column segments
    (700, 200, 264, 8, 40, 16, True, torch.float16, 0.0),      # 8 tasks, unmasked (column-split wave grid), fp16
    (26000, 96, 96, 3, 64, 72, True, torch.bfloat16, 0.05),    # > 1.25 residency rounds: the 128-row tiles, per source
])
def test_pq_kernel_multi_source_shapes(geom, lowrank_form):
    """k_pq with SEVERAL activation sources / output gradients (the T > 0 layers whose projection rows do not fit in LDS: Swin-B at
    rank 128, the r = 64 / 256 points of the 8-task sweep) forced on shapes off its tile grid: all outputs, dX, dX_t and every factor
    gradient against the fp64 oracle with the specified mask (the multi-source launches beyond one residency
    round were only ever run by bench.py)."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.lora import MTLoRALinear
    M, K, N, nt, r_s, r_t, use_xt, dtype, p = geom
    tasks = _TASKS8[:nt]
    torch.manual_seed(M + K + nt)
    m = MTLoRALinear(K, N, r={"shared": r_s, **{t: r_t for t in tasks}}, lora_shared_scale=2.0, lora_task_scale={t: 1.5 for t in tasks},
                     lora_dropout=p, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_((torch.randn_like(q) * (0.05 if "lora" in n_ else 0.02)).to(dtype).float())
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    xs_in = [(0.5 * torch.randn(M, K, device=dev())).to(dtype).requires_grad_(True) for _ in range(1 + (nt if use_xt else 0))]
    prev = Fn.set_tuning(projk=3)
    try:
        c0 = Fn._seed_counter
        y, yt = m(xs_in[0], {t: xs_in[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
        Fn._seed_counter = c0
        seed = Fn.next_seed() if p > 0 else 0
        outs = [y] + [yt[t] for t in tasks]
        gys = [torch.randn(M, N, device=dev()).to(dtype) for _ in outs]
        torch.autograd.backward(outs, gys)
    finally:
        Fn.set_tuning(**prev)
    gdev = torch.device("cpu") if M < 5000 else dev()
    keep = O.dropout_keep_mask_t(seed, 0, M, K, p, device=gdev) if p > 0 else None
    P = {k: v.detach().double().to(gdev).requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xo = [x.detach().double().to(gdev).requires_grad_(True) for x in xs_in]
    yo, yto = O.mtlora_linear(xo[0], P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], m.lora_shared_scale,
                              tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                              scale_t=m.lora_task_scale, x_tasks={t: xo[1 + i] for i, t in enumerate(tasks)} if use_xt else None,
                              keep_mask=keep, p=p)
    torch.autograd.backward([yo] + [yto[t] for t in tasks], [g.double().to(gdev) for g in gys])
    for i, (a, b) in enumerate(zip(outs, [yo] + [yto[t] for t in tasks])):
        assert_close(a, b.detach(), dtype, f"y[{i}]")
    for i, x in enumerate(xs_in):
        assert_close(x.grad, xo[i].grad, dtype, f"dx[{i}]")
    for n_, q in m.named_parameters():
        if q.requires_grad:
            assert_close(q.grad, P[n_].grad, dtype, f"grad {n_}")


def test_full_size_attention_windows_vs_oracle():
    """window attention at the full stage-0 size (B = 32, 112 x 112, 3 heads, shifted): windows are independent, so the
    first and last image of the batch must match the oracle run on those two images alone (forward and dqkv)."""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = 32, 112, 112, 3, 7, 3
    C, N = nH * 32, ws * ws
    dtype = torch.bfloat16
    torch.manual_seed(2)
    qkv = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype).requires_grad_(True)
    bias = (torch.randn(nH, N, N, device=dev()) * 0.5)
    ids = _regions(H, W, ws, shift).to(dev())
    scale = 32 ** -0.5
    meta = Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=scale)
    out = Fn.WindowAttentionFn.apply(meta, qkv, bias, None, ids)
    sel = [0, B - 1]
    g = torch.zeros_like(out)
    g[sel] = torch.randn(2, H, W, C, device=dev()).to(dtype)
    out.backward(g)
    q64 = qkv.detach()[sel].double().cpu().requires_grad_(True)
    win = O.roll_and_window_partition(q64, shift, ws).reshape(-1, N, 3 * C)
    core = O.window_attention_core(win, bias.double().cpu(), O.shifted_window_mask(H, W, ws, shift).double(), nH, scale)
    ref = O.window_merge_and_roll(core.reshape(-1, ws, ws, C), shift, ws, H, W)
    assert_close(out[sel], ref, dtype, "attn out (2 of 32 images)")
    ref.backward(g[sel].double().cpu())
    assert_close(qkv.grad[sel], q64.grad, dtype, "dqkv")
    assert qkv.grad[1:B - 1].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------
# whole model: backbone + Downsampler + HRNet heads + losses through every custom path vs the oracle's full model
# ------------------------------------------------------------------------------------------------
def test_full_model_loss_and_gradients_vs_oracle():
    """MultiTaskSwin (HIP linears / attention / LN / residual, concat-upsample head input, split-reduction head linears,
    fused BatchNorm+ReLU, fused upsample+loss) against oracle.full_model + multi_task_loss in fp64 on the same
    parameters and batch: loss, per-task losses and the gradients of backbone AND head parameters (fp32, train-mode
    BatchNorm statistics, dropout / DropPath off so both sides are deterministic)."""
    from mtlora_amd import mtl_harness as H
    tasks = ["semseg", "normals", "sal", "human_parts"]
    model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=3,
                          DROPOUT=[0.0] * 4).to(dev())
    model.train()
    crit = H.MultiTaskLoss(tasks)
    img, tg = H.synthetic_batch(2, 224, tasks, seed=5, device=dev())
    loss, per = crit.forward_low(model(img, upsample=False), tg)
    loss.backward()
    # oracle on the CPU, fp64, same state dict
    cfg = O.swin_t_cfg(img_size=224, tasks=tasks, r_shared=16, r_task=4, depths=(2, 2, 2, 2), drop_path_rate=0.0, dropout=0.0)
    sd = model.state_dict()
    P = {k: v.detach().double().cpu().clone() for k, v in sd.items()}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    for k in P:
        if k in trainable:
            P[k].requires_grad_(True)
    # running statistics were updated by the forward above; the oracle's train-mode BN only reads batch statistics
    out = O.full_model(P, img.double().cpu(), cfg, train=True, rng=torch.Generator().manual_seed(0))
    rl, rper = O.multi_task_loss(out, {t: v.double().cpu() for t, v in tg.items()}, tasks)
    rl.backward()
    assert abs(loss.item() - rl.item()) <= 1e-3 * abs(rl.item()), (loss.item(), rl.item())
    for t in tasks:
        assert abs(per[t].item() - rper[t].item()) <= 1e-3 * max(1.0, abs(rper[t].item())), t
    named = dict(model.named_parameters())
    gmax = max(P[n].grad.abs().max().item() for n in trainable if P[n].grad is not None)
    checked = 0
    for n in sorted(trainable):
        g, r = named[n].grad, P[n].grad
        if r is None:
            assert g is None, n
            continue
        assert g is not None, n
        if n.endswith("last_layer.0.bias"):
            # the bias in front of a BatchNorm: its gradient is the column sum of the BN-backward output, analytically 0;
            # both sides only hold rounding noise
            assert g.abs().max().item() <= 1e-4 * gmax and r.abs().max().item() <= 1e-4 * gmax, n
            continue
        scale = max(r.abs().max().item(), 1e-6 * gmax)
        e = (g.double().cpu() - r).abs() / scale
        err = e.max().item()
        if n.startswith("decoders.") and err > 5e-3:
            # head tensors sit behind ReLU / train-mode BatchNorm: a pre-activation within fp32 rounding of 0 may take the other
            # branch than in fp64 and moves ONE row / column of the weight gradient (tools/debug_bn.py, tools/debug_head_grad.py:
            # the same tensor is at 4e-4 or 8e-3 depending on which fp32 GEMM produced the layer input).  Accept such a flip:
            # <= 1 % of the elements beyond the bound, none beyond 10x
            assert (e > 5e-3).double().mean().item() <= 0.01 and err <= 5e-2, (n, err, (e > 5e-3).double().mean().item())
        else:
            assert err <= 5e-3, (n, err)
        checked += 1
    assert checked > 200


def test_task_streams_match_single_stream():
    """MultiTaskSwin runs the per-task Downsampler + head + fused-loss chains on one side stream per task: loss and every
    gradient must equal the single-stream execution bit for bit (same kernels, same order within a chain), twice in a row
    (the second step reuses the caching allocator's blocks across streams)."""
    from mtlora_amd import mtl_harness as H
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=7, device=dev())
    res = []
    for conc in (False, True):
        model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=3,
                              DROPOUT=[0.0] * 4).to(dev()).train()
        crit = H.MultiTaskLoss(tasks)
        steps = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss, _ = crit.combine(model(img, upsample=False, per_task_fn=lambda t, lo: crit.task_low(t, lo, tg[t]),
                                             concurrent=conc))
            loss.backward()
            torch.cuda.synchronize()
            steps.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
        res.append(steps)
    for (l0, g0), (l1, g1) in zip(*res):
        assert torch.equal(l0, l1)
        assert g0.keys() == g1.keys() and len(g0) > 200
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_pack_table_equals_per_call_pack(dtype):
    """mtlora_linear_pack_table over a two-layer table writes, for each dtype of the host ladder, exactly the bytes that
    mtlora_linear_pack writes layer by layer (smallest shapes: one layer with task factors, one with the shared factor only)."""
    import ctypes
    from mtlora_amd import _lib
    from mtlora_amd import functional as Fn
    torch.manual_seed(17)
    entries, want = [], []
    for K, N, r_s, r_t in ((8, 8, 4, (4, 4)), (16, 24, 8, ())):
        meta = Fn.LinearMeta(K=K, N=N, r_s=r_s, r_t=r_t, scale_s=2.0, scale_t=tuple(0.5 + t for t in range(len(r_t))), mode=0,
                             has_x_tasks=bool(r_t), dropout_p=0.0, seed=0, dtype=dtype)
        A_s, B_s = torch.randn(r_s, K, device=dev()), torch.randn(N, r_s, device=dev())
        A_t, B_t = [torch.randn(r, K, device=dev()) for r in r_t], [torch.randn(N, r, device=dev()) for r in r_t]
        nbytes = Fn.packed_bytes(meta)
        ref, buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev()), torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        d = meta.desc(1)
        _lib.check(_lib.lib().mtlora_linear_pack(ctypes.byref(d), _lib.ptr(A_s), _lib.ptr(B_s), _lib.ptr_array(A_t), _lib.ptr_array(B_t),
                                                 _lib.ptr(ref), nbytes, _lib.stream_ptr()), "mtlora_linear_pack")
        entries.append((meta, A_s, B_s, A_t, B_t, buf))
        want.append(ref)
    Fn.PackTable(entries, dev(), dtype).pack()
    for (*_, buf), ref in zip(entries, want):
        assert bool(ref.any()) and torch.equal(buf, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,Na,Nb", [(20000, 24, 1080), (4099, 8, 264), (70001, 136, 40), (300, 64, 256), (0, 8, 8)])
def test_gemm_tn_vs_torch(dtype, M, Na, Nb):
    """mtlora_gemm_tn: out = a^T b (the narrow-output weight gradient), ragged M, several a-tiles, empty input."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(M + Na)
    a = torch.randn(M, Na, device=dev()).to(dtype)
    b = torch.randn(M, Nb, device=dev()).to(dtype)
    out = Fn.gemm_tn(a, b)
    ref = a.double().cpu().t() @ b.double().cpu()
    assert out.dtype == torch.float32 and out.shape == (Na, Nb)
    tol = 1e-3 * max(1.0, math.sqrt(M))  # fp32 accumulation of M products of unit-variance terms
    assert (out.double().cpu() - ref).abs().max().item() <= tol
    assert torch.equal(out, Fn.gemm_tn(a, b))  # deterministic


@pytest.mark.parametrize("shape", [(32768, 72, 40), (32768, 72, 136), (16384, 1080, 24)])
@pytest.mark.parametrize("autocast", [False, True])
def test_split_reduction_linear_vs_f_linear(autocast, shape):
    """functional.linear_big_m (forward / dX through the rank-0 k_nt path, weight gradient as the library's TN reduction
    for narrow outputs or a batched GEMM over row chunks, two-stage bias sum) == F.linear, values and gradients;
    feeds_batchnorm=True returns an exactly zero bias gradient."""
    from mtlora_amd import functional as Fn
    M, K, N = shape
    torch.manual_seed(4)
    x = torch.randn(M, K, device=dev(), requires_grad=True)
    w = (torch.randn(N, K, device=dev()) * 0.1).requires_grad_(True)
    b = torch.randn(N, device=dev()).requires_grad_(True)
    gy = torch.randn(M, N, device=dev())
    dt = torch.bfloat16 if autocast else torch.float32
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = Fn.linear_big_m(x, w, b)
    assert y.dtype == dt
    y.backward(gy.to(dt))
    xr, wr, br = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(gy.double().cpu())
    assert_close(y, yr, dt, "y")
    assert_close(x.grad, xr.grad, dt, "dx")
    assert_close(w.grad, wr.grad, dt, "dw")
    assert_close(b.grad, br.grad, dt, "db")
    b.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        Fn.linear_big_m(x, w, b, feeds_batchnorm=True).backward(gy.to(dt))
    assert b.grad is not None and b.grad.abs().max().item() == 0.0


# ---- small deterministic reductions (csrc/reduce.hip): the ATen sums they replace issue device memsets
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(100352, 8), (100352, 24), (401408, 96), (1000, 1080), (7, 8), (3001, 4096)])
def test_column_sum_vs_torch(shape, dtype):
    from mtlora_amd import functional as Fn
    M, N = shape
    torch.manual_seed(M + N)
    g = torch.randn(M, N, device=dev()).to(dtype)
    out = Fn.column_sum(g)
    ref = g.double().sum(0)
    assert out.dtype == torch.float32 and out.shape == (N,)
    scale = g.double().abs().sum(0).max().item()
    assert (out.double() - ref).abs().max().item() <= 2e-6 * scale + 1e-6
    assert torch.equal(out, Fn.column_sum(g))  # deterministic


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32 * 448 * 448, 3 * 32 * 448 * 448, 1003, 4])
def test_label_stat_vs_torch(n):
    from mtlora_amd import functional as Fn
    torch.manual_seed(n)
    lab = torch.randint(0, 21, (n,), device=dev()).float()
    lab[torch.rand(n, device=dev()) < 0.1] = 255.0
    cnt = Fn.label_stat(lab, 0, 255.0)
    assert cnt.item() == (lab != 255.0).sum().float().item()  # the exact count, rounded once to fp32 (what .sum().float() gave)
    sal = torch.rand(n, device=dev())
    w = Fn.label_stat(sal, 1, 255.0)
    ref = (1.0 - (sal >= 0.5).double()).mean().item()
    assert abs(w.item() - ref) <= 1e-6


@pytest.mark.gpu
def test_droppath_bulk_draw():
    """functional._DropPathPool: the requests of one announced step become the plan of the next, whose factors come from ONE
    draw (views of one tensor), each in {0, 1/keep} with the right keep rate; a deviating request falls back to its own draw."""
    from mtlora_amd import functional as Fn
    d = dev()
    reqs = [(1, 64, 0.9), (5, 64, 0.8), (1, 64, 0.75), (5, 64, 0.5)]
    Fn.droppath_begin_step(d)
    first = [Fn.droppath_scale(n, B, k, d) for n, B, k in reqs]  # recorded, drawn one by one
    Fn.droppath_end_step()
    assert len({t.untyped_storage().data_ptr() for t in first}) == len(first)
    torch.manual_seed(3)
    Fn.droppath_begin_step(d)
    second = [Fn.droppath_scale(n, B, k, d) for n, B, k in reqs]
    Fn.droppath_end_step()
    assert len({t.untyped_storage().data_ptr() for t in second}) == 1  # one bulk tensor
    for (n, B, k), t in zip(reqs, second):
        assert t.shape == (n, B) and t.dtype == torch.float32
        assert bool(((t == 0) | ((t - 1.0 / k).abs() < 1e-6)).all())
    torch.manual_seed(3)
    Fn.droppath_begin_step(d)
    again = [Fn.droppath_scale(n, B, k, d) for n, B, k in reqs]
    Fn.droppath_end_step()
    assert all(torch.equal(a, b) for a, b in zip(second, again))  # reproducible under the global generator
    # keep rate over many draws
    Fn.droppath_begin_step(d)
    rate = torch.stack([Fn.droppath_scale(5, 64, 0.8, d) if i == 1 else Fn.droppath_scale(*reqs[i][:2], reqs[i][2], d)
                        for i in range(4)][1:2]).ne(0).float().mean().item()
    Fn.droppath_end_step()
    assert 0.6 < rate < 0.95
    # a deviating request (other batch) gets its own draw and the plan is re-recorded
    Fn.droppath_begin_step(d)
    odd = Fn.droppath_scale(2, 32, 0.9, d)
    Fn.droppath_end_step()
    assert odd.shape == (2, 32)
    Fn.droppath_begin_step(d)
    Fn.droppath_end_step()  # leave an empty plan behind for the other tests
