"""The folded autograd nodes of mtlora_amd/functional.py on the paths no other test enters: the LayerNorm fork with one output
unused, the merged-streams node in both forms (with and without a residual), the big-M linear with either forward, and the
factor-gradient side stream of the Mlp with implicit task hiddens.  References: ATen in fp64; tolerances of the suite
(1e-3 fp32, 1e-2 bf16, relative to max |ref|)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import _mlp_with_tasks, assert_close, dev  # noqa: F401  (the suite's helpers and tolerance table)

pytestmark = pytest.mark.gpu


def _ln_params(C):
    w = (1.0 + 0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    b = (0.1 * torch.randn(C, device=dev())).requires_grad_(True)
    return w, b


def _grad_or_zero(p):
    return torch.zeros_like(p) if p.grad is None else p.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("use", ["skip", "y", "both"])
def test_layer_norm_fork_with_an_unused_output(dtype, use):
    """LayerNormFn's fork form (x_skip, y) = (x, LayerNorm(x)) with only the skip output used (the normalised output's gradient is
    absent: dx is the skip gradient, dgamma = dbeta = 0), only the normalised output used, and both: dx, dgamma, dbeta against fp64."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(11)
    B, Lt, C = 2, 16, 32
    x = torch.randn(B, Lt, C, device=dev()).to(dtype).requires_grad_(True)
    w, b = _ln_params(C)
    g_skip, g_y = torch.randn(B, Lt, C, device=dev()).to(dtype), torch.randn(B, Lt, C, device=dev()).to(dtype)
    skip, y = Fn.LayerNormFn.apply(x, w, b, 1e-5, dtype, None, True)
    assert skip.dtype == x.dtype and y.dtype == dtype and torch.equal(skip, x)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    y64 = F.layer_norm(x64, (C,), w64, b64, 1e-5)
    assert_close(y, y64, dtype, "y")
    outs, gs, outs64, gs64 = [], [], [], []
    if use in ("skip", "both"):
        outs, gs, outs64, gs64 = outs + [skip], gs + [g_skip], outs64 + [x64 * 1.0], gs64 + [g_skip.double()]
    if use in ("y", "both"):
        outs, gs, outs64, gs64 = outs + [y], gs + [g_y], outs64 + [y64], gs64 + [g_y.double()]
    torch.autograd.backward(outs, gs)
    torch.autograd.backward(outs64, gs64)
    assert_close(x.grad, x64.grad, dtype, "dx")
    if use == "skip":
        assert torch.equal(x.grad, g_skip)
        assert not _grad_or_zero(w).any() and not _grad_or_zero(b).any()
    else:
        assert_close(w.grad, w64.grad, dtype, "dgamma")
        assert_close(b.grad, b64.grad, dtype, "dbeta")


def _merge_gather(x, H, W):
    B, _, C = x.shape
    return x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("use_scale", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n", [2, 5])
def test_merged_streams_node_with_and_without_a_residual(n, residual, use_scale, dtype):
    """ResidualMergeNormStreamsFn in both forms -- n streams normalised as they are (``mtlora_layernorm_multi_*``) and
    res_k + scale[k] * branch_k formed first (``mtlora_residual_layernorm_streams_*``) -- against the per-stream fp64 computation
    (residual, 2x2 gather, LayerNorm): stacked output, every input gradient, dgamma / dbeta.  With a residual and n = 5 the node must
    also reproduce five calls of itself with one stream each bit for bit (outputs and input gradients; the parameter gradients are
    sums over the streams in another order: tolerance).  Without branches a scale has nothing to apply to and is ignored."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(7 * n + 1)
    B, H, W, C = 2, 4, 4, 16
    w, b = _ln_params(4 * C)
    res = [torch.randn(B, H * W, C, device=dev()).to(dtype).requires_grad_(True) for _ in range(n)]
    brs = [torch.randn(B, H * W, C, device=dev()).to(dtype).requires_grad_(True) for _ in range(n)] if residual else []
    scale = ((torch.rand(n, B, device=dev()) < 0.7).float() / 0.7) if use_scale else None
    g = torch.randn(n * B, H * W // 4, 4 * C, device=dev()).to(dtype)
    st = Fn.ResidualMergeNormStreamsFn.apply(scale, w, b, 1e-5, dtype, H, W, n, *res, *brs)
    assert st.shape == (n * B, H * W // 4, 4 * C) and st.dtype == dtype
    st.backward(g)
    w64, b64 = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    r64 = [t.detach().double().requires_grad_(True) for t in res]
    br64 = [t.detach().double().requires_grad_(True) for t in brs]
    ys = []
    for k in range(n):
        xk = r64[k]
        if residual:
            xk = xk + (br64[k] if scale is None else br64[k] * scale[k].double().view(B, 1, 1))
        ys.append(F.layer_norm(_merge_gather(xk, H, W), (4 * C,), w64, b64, 1e-5))
    ref = torch.cat(ys, 0)
    ref.backward(g.double())
    assert_close(st, ref, dtype, "stacked output")
    for k in range(n):
        assert_close(res[k].grad, r64[k].grad, dtype, f"d_res{k}")
        if residual:
            if scale is not None and not scale[k].any():  # every sample of the stream dropped: the gradient is exactly zero
                assert not brs[k].grad.any()
            else:
                assert_close(brs[k].grad, br64[k].grad, dtype, f"d_branch{k}")
    assert_close(w.grad, w64.grad, dtype, "dgamma")
    assert_close(b.grad, b64.grad, dtype, "dbeta")
    if residual and n == 5:
        w1, b1 = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        for k in range(n):
            rk, bk = res[k].detach().clone().requires_grad_(True), brs[k].detach().clone().requires_grad_(True)
            one = Fn.ResidualMergeNormStreamsFn.apply(None if scale is None else scale[k:k + 1].contiguous(), w1, b1, 1e-5, dtype, H, W, 1,
                                                      rk, bk)
            assert torch.equal(one, st[k * B:(k + 1) * B]), k
            one.backward(g[k * B:(k + 1) * B])
            assert torch.equal(rk.grad, res[k].grad) and torch.equal(bk.grad, brs[k].grad), k
        assert_close(w1.grad, w.grad.double(), dtype, "dgamma (five single-stream calls)")
        assert_close(b1.grad, b.grad.double(), dtype, "dbeta (five single-stream calls)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("zero_bias_grad", [False, True])
@pytest.mark.parametrize("rows,pad_rows", [(5, 3), (72, 0)])
@pytest.mark.parametrize("via_knt", [False, True])
def test_big_linear_node_both_forwards(via_knt, rows, pad_rows, zero_bias_grad, dtype):
    """BigLinearFn through hipBLASLt and through the library's rank-0 kernel (``via_knt``), M = 1024 in four row chunks, the weight's
    24 columns scattered into the input's 32 by ``col_index``, N = 8 (5 rows padded by 3: dW through ``gemm_tn`` on the k_nt path) and
    N = 72 (past the N <= 64 branch): y, dX, dW and db against F.linear in fp64 on the laid-out weight; with ``zero_bias_grad`` the bias
    gradient is the promised exact zero."""
    from mtlora_amd import functional as Fn
    torch.manual_seed(rows + 3)
    M, Kw, Kx, S = 1024, 24, 32, 4
    x = torch.randn(M, Kx, device=dev()).to(dtype).requires_grad_(True)
    weight = (0.2 * torch.randn(rows, Kw, device=dev())).requires_grad_(True)
    bias = (0.2 * torch.randn(rows, device=dev())).requires_grad_(True)
    col_index = torch.randperm(Kx, device=dev())[:Kw].sort().values
    gy = torch.randn(M, rows + pad_rows, device=dev()).to(dtype)
    y = Fn.BigLinearFn.apply(x, weight, bias, S, zero_bias_grad, dtype, via_knt, col_index, Kx, pad_rows)
    assert y.shape == (M, rows + pad_rows) and y.dtype == dtype
    y.backward(gy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, weight, bias))
    y64 = F.pad(F.linear(x64[:, col_index], w64, b64), (0, pad_rows))
    y64.backward(gy.double())
    assert_close(y, y64, dtype, "y")
    assert_close(x.grad, x64.grad, dtype, "dX")
    assert weight.grad.shape == weight.shape and weight.grad.dtype == weight.dtype
    assert_close(weight.grad, w64.grad, dtype, "dW")
    assert bias.grad.shape == bias.shape
    if zero_bias_grad:
        assert not bias.grad.any()
    else:
        assert_close(bias.grad, b64.grad, dtype, "db")


def _factor_grads(mod):
    return {n: p.grad.detach().clone() for n, p in mod.named_parameters() if "lora_" in n and p.grad is not None}


class _CountingStream(torch.cuda.Stream):
    """a side stream that counts the forks onto it: the runner makes it wait for one event per backward call it hands phase 2 to"""
    forks = 0

    def wait_event(self, event):
        _CountingStream.forks += 1
        return super().wait_event(event)


def _with_side_stream(step, mod):
    """factor gradients of ``step()`` (one forward + backward of ``mod``) without and with the side stream installed, the number of
    Parameters left pending on it and the number of backward calls that forked onto it"""
    from mtlora_amd import functional as Fn
    side = _CountingStream()
    out = []
    keep_m = Fn._FACTOR_MIN_M
    try:
        Fn._FACTOR_MIN_M = 0  # (the row threshold would keep these small layers on the main stream)
        for use_side in (False, True):
            mod.zero_grad(set_to_none=True)
            Fn.factor_stream_joined()
            Fn.set_factor_stream(side if use_side else None)
            try:
                Fn._seed_counter = 700
                _CountingStream.forks = 0
                step()
                marked = len(Fn._side_pending)
            finally:
                Fn.set_factor_stream(None)
            torch.cuda.current_stream().wait_stream(side)
            Fn.factor_stream_joined()
            torch.cuda.synchronize()
            out.append((_factor_grads(mod), marked, _CountingStream.forks))
    finally:
        Fn._FACTOR_MIN_M = keep_m
    return out


@pytest.mark.parametrize("uses", [1, 2])
def test_side_stream_runner_linear(uses):
    """one MTLoRALinear (M = 64, K = 32, N = 64, r_s = 8, r_t = (4, 4)) with the factor-gradient side stream: its six factor gradients
    bit-equal to the single-stream ones; used twice in one graph, the second backward call finds the factors pending from the same pass
    and stays on the main stream (all six stay marked)."""
    from mtlora_amd.lora import MTLoRALinear
    torch.manual_seed(21)
    tasks = ["a", "b"]
    m = MTLoRALinear(32, 64, r={"shared": 8, "a": 4, "b": 4}, lora_shared_scale=2.0, lora_task_scale={"a": 1.5, "b": 1.5},
                     lora_dropout=0.0, tasks=tasks).to(dev())
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n_ else 0.02))
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    m.train()
    xs = [[torch.randn(64, 32, device=dev()).requires_grad_(True) for _ in range(3)] for _ in range(uses)]

    def step():
        loss = 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for x, xa, xb in xs:
                y, yt = m(x, {"a": xa, "b": xb})
                loss = loss + (y.float() ** 2).mean() + sum((v.float() ** 2).mean() for v in yt.values())
        loss.backward()

    (ref, n0, f0), (got, n1, f1) = _with_side_stream(step, m)
    assert f0 == 0 and f1 == 1  # one fork per pass: with two uses, the later backward call stays on the main stream
    assert n0 == 0 and n1 == 6 and ref.keys() == got.keys() and len(ref) == 6
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


@pytest.mark.parametrize("uses", [1, 2])
@pytest.mark.parametrize("hidden", [64, 128])
def test_side_stream_runner_mlp(hidden, uses):
    """the task-enabled Mlp (M = 64, K = 32, r_s = 8, r_t = (4, 4)) with the factor-gradient side stream: hidden 128 runs as ONE
    ``MlpHidFn`` node (fc2(1), hid, fc1(1) on the main stream | fc2(2), fc1(2) on the side stream), hidden 64 is below the 128-column
    granule of the implicit-hiddens kernels and runs as two MTLoRALinearFn nodes.  Either way the twelve factor gradients are
    bit-equal to the single-stream ones, and a second use in the same graph stays on the main stream (all twelve stay marked)."""
    from mtlora_amd import functional as Fn
    tasks = ["a", "b"]
    mlp = _mlp_with_tasks(tasks, 32, hidden, 8, 4, 0.0, seed=31)
    xs = [[torch.randn(64, 32, device=dev()).requires_grad_(True) for _ in range(3)] for _ in range(uses)]
    seen = []
    orig = Fn.MlpHidFn.forward

    def spy(ctx, *a):
        seen.append(1)
        return orig(ctx, *a)

    def step():
        loss = 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for x, xa, xb in xs:
                y, yt = mlp(x, {"a": xa, "b": xb})
                loss = loss + (y.float() ** 2).mean() + sum((v.float() ** 2).mean() for v in yt.values())
        loss.backward()

    Fn.MlpHidFn.forward = staticmethod(spy)
    try:
        (ref, n0, f0), (got, n1, f1) = _with_side_stream(step, mlp)
    finally:
        Fn.MlpHidFn.forward = staticmethod(orig)
    assert len(seen) == (2 * uses if hidden == 128 else 0)
    assert f0 == 0 and f1 == (1 if hidden == 128 else 2)  # one fork per node and pass (fc1 and fc2 are nodes of their own at hidden 64)
    assert n0 == 0 and n1 == 12 and ref.keys() == got.keys() and len(ref) == 12
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
