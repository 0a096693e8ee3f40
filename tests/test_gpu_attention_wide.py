"""Window attention for 64 < N = ws*ws <= 144 (window sizes 9..12: csrc/attention_wide.h) against the fp64 oracle, at the
project's tolerances (test_gpu_kernels.TOL, multiplier 1): core in both layouts and all three mask forms, key / query padding,
run-to-run determinism, a window-12 SwinTransformerBlock per layer and as one block call, and the shared gather constant."""
import pytest
import torch

from oracle import mtlora_oracle as O
from test_gpu_kernels import TOL, _regions, assert_close, dev, rel_err  # noqa: F401  (the suite's helpers and tolerance table)

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5


def _meta(B, H, W, nH, ws, shift):
    from mtlora_amd import functional as Fn
    return Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=SCALE)


def _oracle(qkv, bias, mask, nH, ws, shift, H, W):
    """(out, q64, b64, window-ordered qkv, core) of the fp64 oracle: roll + partition -> core -> merge + roll"""
    C, N = nH * 32, ws * ws
    q64 = qkv.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True)
    win = O.roll_and_window_partition(q64, shift, ws).reshape(-1, N, 3 * C)
    core = O.window_attention_core(win, b64, None if mask is None else mask.double(), nH, SCALE)
    ref = O.window_merge_and_roll(core.reshape(-1, ws, ws, C), shift, ws, H, W)
    return ref, q64, b64, win, core


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [
    # (B, H, W, heads, ws, shift)
    (2, 24, 24, 3, 12, 6), (2, 24, 24, 3, 12, 0), (1, 20, 30, 2, 10, 3), (1, 9, 18, 1, 9, 4), (3, 12, 12, 6, 12, 0),
    (1, 22, 11, 2, 11, 5),
    # 128 windows over 8 heads: 32 backward / 64 forward workgroups per head, i.e. every workgroup walks its persistent loop 2..4
    # times over masked and unmasked windows (dbias accumulates across them, the images, tables and statistics are reused)
    (8, 48, 48, 8, 12, 6),
])
def test_wide_attention_core_vs_oracle(cfg, dtype):
    """the form of test_attention_core_vs_oracle: image layout + region ids, window layout + dense mask, image layout + dense mask"""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = cfg
    C, N = nH * 32, ws * ws
    torch.manual_seed(H * W + nH)
    qkv_img = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype).requires_grad_(True)
    bias = (torch.randn(nH, N, N, device=dev()) * 0.5).requires_grad_(True)
    mask = O.shifted_window_mask(H, W, ws, shift)
    mask_d = None if mask is None else mask.to(dev())
    meta = _meta(B, H, W, nH, ws, shift)
    ids = None if mask is None else _regions(H, W, ws, shift).to(dev())
    out = Fn.WindowAttentionFn.apply(meta, qkv_img, bias, None, ids)
    ref, q64, b64, win, core = _oracle(qkv_img, bias, mask, nH, ws, shift, H, W)
    assert_close(out, ref, dtype, "attn out")
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double().cpu())
    assert_close(qkv_img.grad, q64.grad, dtype, "dqkv")
    assert_close(bias.grad, b64.grad, dtype, "dbias")
    # window-major layout, dense mask
    qkv_win = win.detach().to(dev()).to(dtype).contiguous().requires_grad_(True)
    nW = 1 if mask is None else mask.shape[0]
    meta_w = Fn.AttnMeta(B=qkv_win.shape[0] // nW, H=ws, W=ws * nW, window_size=ws, shift=0, num_heads=nH, head_dim=32,
                         image_layout=False, scale=SCALE)
    out_w = Fn.WindowAttentionFn.apply(meta_w, qkv_win, bias.detach(), mask_d, None)
    assert_close(out_w, core, dtype, "attn out (windows)")
    if mask is not None:  # dense mask, image layout, forward + backward
        q2 = qkv_img.detach().clone().requires_grad_(True)
        b2 = bias.detach().clone().requires_grad_(True)
        out_d = Fn.WindowAttentionFn.apply(meta, q2, b2, mask_d, None)
        assert_close(out_d, ref, dtype, "attn out (dense mask)")
        out_d.backward(g)
        assert_close(q2.grad, q64.grad, dtype, "dqkv (dense mask)")
        assert_close(b2.grad, b64.grad, dtype, "dbias (dense mask)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ws", [9, 12])
def test_wide_attention_padding(ws, dtype):
    """keys 81..159 / 144..159 of the padded tiles must carry exactly zero probability and padded queries must not reach dK / dV /
    dbias: every score is large and positive (q = k > 0, bias +15 as in test_attention_large_relative_bias_vs_oracle), so a padded
    key entering the softmax with score 0 + garbage bias -- or 'a large negative bias' added to it -- would move the row sums.
    dbias is written into a poisoned buffer through the C ABI: all N*N entries of every head, none left."""
    import ctypes
    from mtlora_amd import _lib as L
    from mtlora_amd import functional as Fn
    B, H, W, nH, shift = 2, 2 * ws, ws, 2, ws // 2
    C, N = nH * 32, ws * ws
    torch.manual_seed(ws)
    qkv = (torch.rand(B, H, W, 3 * C, device=dev()) * 0.5 + 0.75).to(dtype).requires_grad_(True)
    bias = (15.0 + torch.randn(nH, N, N, device=dev())).requires_grad_(True)
    mask = O.shifted_window_mask(H, W, ws, shift)
    ids = _regions(H, W, ws, shift).to(dev())
    meta = _meta(B, H, W, nH, ws, shift)
    out = Fn.WindowAttentionFn.apply(meta, qkv, bias, None, ids)
    ref, q64, b64, _, _ = _oracle(qkv, bias, mask, nH, ws, shift, H, W)
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double().cpu())
    assert_close(out, ref, dtype, "attn out (padding)")
    assert_close(qkv.grad, q64.grad, dtype, "dqkv (padding)")
    assert_close(bias.grad, b64.grad, dtype, "dbias (padding)")
    # poisoned dbias / dqkv buffers straight through the entry point
    d = meta.desc(dtype)
    lib = L.lib()
    sb = lib.mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev())
    poison = -12345.678
    dbias = torch.full((nH, N, N), poison, device=dev())
    dqkv = torch.full_like(qkv.detach(), 777.0)
    qc, bc, gc = qkv.detach().contiguous(), bias.detach().contiguous(), g.contiguous()
    st = lib.mtlora_window_attn_bwd(ctypes.byref(d), L.ptr(qc), L.ptr(bc), None, L.ptr(ids), L.ptr(gc), L.ptr(dqkv),
                                    L.ptr(dbias), L.ptr(scratch), sb, L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    assert int((dbias == poison).sum()) == 0 and bool(torch.isfinite(dbias).all())
    assert torch.equal(dbias, bias.grad)
    assert torch.equal(dqkv, qkv.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", [(4, 24, 36, 3, 12, 6), (8, 48, 48, 8, 12, 6), (6, 36, 27, 5, 9, 4)])
def test_wide_attention_backward_is_deterministic(geom, dtype):
    """(the second and third shapes have more windows than resident workgroups per head: 128 over 32, 72 over 51 in the backward)"""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = geom
    C, N = nH * 32, ws * ws
    torch.manual_seed(3)
    qkv = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype)
    bias = torch.randn(nH, N, N, device=dev()) * 0.5
    ids = _regions(H, W, ws, shift).to(dev())
    g = None
    runs = []
    for _ in range(2):
        q, b = qkv.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        out = Fn.WindowAttentionFn.apply(_meta(B, H, W, nH, ws, shift), q, b, None, ids)
        g = torch.randn_like(out) if g is None else g
        out.backward(g)
        runs.append((out.detach(), q.grad, b.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _oracle_block(blk, x, ws, shift, nH, H, W):
    P = {"b." + n: p.detach().double().cpu().requires_grad_(True) for n, p in blk.named_parameters()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    y, _ = O.swin_block(P, "b", x64, H, W, nH, ws, shift, None, 0, mt)
    return y, x64, P


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shift", [6, 0])
def test_window12_block_vs_oracle(shift, dtype):
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerBlock
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    blk = SwinTransformerBlock(64, (24, 24), 2, window_size=12, shift_size=shift, lora=False, tasks=None, mtlora=mt, layer_idx=0)
    O.det_fill_(blk.named_parameters())
    blk = blk.to(dev()).eval()
    x = O.det_tensor(f"w12.{shift}.x", (2, 24 * 24, 64), 1.0).to(dev()).float().requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        y = blk(x)[0]
    ref, x64, P = _oracle_block(blk, x, 12, shift, 2, 24, 24)
    assert_close(y, ref, dtype, "y")
    gy = O.det_tensor(f"w12.{shift}.gy", y.shape, 1.0)
    (y.float() * gy.to(dev())).sum().backward()
    (ref * gy.double()).sum().backward()
    assert_close(x.grad, x64.grad, dtype, "dx")
    for n, p in blk.named_parameters():
        if not p.requires_grad:  # (frozen pretrained weights)
            continue
        assert p.grad is not None and P["b." + n].grad is not None, n
        assert_close(p.grad, P["b." + n].grad, dtype, f"grad {n}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_window12_block_call_matches_per_layer_calls(dtype):
    """window-12 blocks (shift 0 and 6) through ONE library call per block and direction (functional.SwinBlockRunFn) are bit-identical
    to the per-layer autograd Functions: same launches in the same order, as test_block_call_matches_per_layer_calls has it for 7"""
    from mtlora_amd import functional as Fn
    from mtlora_amd import swin_transformer_mtlora as S
    tasks = ["semseg", "normals"]
    mt = O.mtlora_config(tasks, r_shared=8, r_task=4, dropout=0.0)
    layer = S.BasicLayer(dim=64, input_resolution=(24, 24), depth=3, num_heads=2, window_size=12, tasks=tasks, mtlora=mt, layer_idx=0)
    O.det_fill_(layer.named_parameters())
    for n, p in layer.named_parameters():  # frozen pretrained weights, as mark_only_lora_as_trainable leaves them (the one-call path
        if ".linear." in n:                # keeps a block with trainable dense weights on the per-layer Functions)
            p.requires_grad_(False)
    layer = layer.to(dev()).train()
    x0 = O.det_tensor("w12.layer.x", (2, 24 * 24, 64), 1.0).to(dev()).float()
    calls = [0]
    orig = Fn.SwinBlockRunFn.forward

    def counting(ctx, cl, *a):
        calls[0] += len(cl)
        return orig(ctx, cl, *a)

    def run():
        layer.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
        with ctx:
            y, yt = layer(x)
        (y.float().square().sum() + sum(v.float().square().sum() for v in yt.values())).backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters() if p.grad is not None]

    keep = S.set_fused_blocks(False)
    Fn.SwinBlockRunFn.forward = staticmethod(counting)
    try:
        ref = run()
        assert calls[0] == 0
        S.set_fused_blocks(True)
        got = run()
        assert calls[0] == 2  # blocks 0 (shift 0) and 1 (shift 6); the last block carries the task outputs
    finally:
        Fn.SwinBlockRunFn.forward = staticmethod(orig)
        S.set_fused_blocks(keep)
    assert len(ref) == len(got)
    for a, b in zip(ref, got):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_window12_bias_gather_constant_is_shared():
    """two ws-12 attention modules on one device share their (2ws-1)^2 x N^2 fp32 gather matrix (44 MB): building both costs less
    than 1.5x one matrix, the bias values are the table's own, and d table (one product with the shared matrix) matches the oracle"""
    from mtlora_amd import swin_transformer_mtlora as S
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    S._RPI_ONEHOT.clear()
    torch.cuda.synchronize()
    one = 23 * 23 * 144 * 144 * 4
    mods = [S.WindowAttention(64, (12, 12), 2, mtlora=mt, layer_idx=0).to(dev()) for _ in range(2)]
    with torch.no_grad():
        for k, m in enumerate(mods):
            m.relative_position_bias_table.copy_(O.det_tensor(f"w12.table.{k}", m.relative_position_bias_table.shape, 1.0))
    before = torch.cuda.memory_allocated()
    biases = [m.dense_bias() for m in mods]
    grown = torch.cuda.memory_allocated() - before - sum(b.numel() * 4 for b in biases)
    assert grown < 1.5 * one, (grown, one)
    assert mods[0]._rpi_onehot is mods[1]._rpi_onehot
    for m, b in zip(mods, biases):
        t64 = m.relative_position_bias_table.detach().double().cpu().requires_grad_(True)
        ref = O.dense_relative_bias(t64, 12)
        assert torch.equal(b.detach().cpu(), ref.detach().float())
        g = O.det_tensor("w12.dbias", b.shape, 1.0)
        b.backward(g.to(dev()))
        ref.backward(g.double())
        assert rel_err(m.relative_position_bias_table.grad, t64.grad) <= 1e-6
