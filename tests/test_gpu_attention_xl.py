"""Window attention for 144 < N = ws*ws <= 256 (window sizes 13..16: csrc/attention_xl.h) against the fp64 oracle, at the project's
tolerances (test_gpu_kernels.TOL, multiplier 1): core in both layouts and all three mask forms, key / query padding, run-to-run
determinism, a window-14 SwinTransformerBlock on the per-layer path, and the bias gather / scatter kernels behind ``dense_bias``."""
import ctypes

import pytest
import torch

from oracle import mtlora_oracle as O
from test_gpu_attention_wide import _meta, _oracle, _oracle_block
from test_gpu_kernels import TOL, _regions, assert_close, dev  # noqa: F401  (the suite's helpers and tolerance table)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", [
    # (B, H, W, heads, ws, shift)
    (1, 26, 13, 2, 13, 6),   # N = 169: 9 valid rows in the last tile
    (2, 28, 28, 3, 14, 7),   # N = 196
    (1, 15, 30, 1, 15, 7),   # N = 225: one row short of a tile
    (1, 32, 32, 2, 16, 8),   # N = 256: no padding at all
    (1, 14, 14, 2, 14, 0),   # the single-window last stage
    # 64 windows per head: the persistent loops and the cross-window dbias accumulation run several rounds over masked and unmasked windows
    (4, 56, 56, 4, 14, 7),
])
def test_xl_attention_core_vs_oracle(cfg, dtype):
    """the form of test_wide_attention_core_vs_oracle: image layout + region ids, window layout + dense mask, image layout + dense mask"""
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
    assert_close(out, ref, dtype, "xl attn out")
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double().cpu())
    assert_close(qkv_img.grad, q64.grad, dtype, "xl dqkv")
    assert_close(bias.grad, b64.grad, dtype, "xl dbias")
    # window-major layout, dense mask
    qkv_win = win.detach().to(dev()).to(dtype).contiguous().requires_grad_(True)
    nW = 1 if mask is None else mask.shape[0]
    meta_w = Fn.AttnMeta(B=qkv_win.shape[0] // nW, H=ws, W=ws * nW, window_size=ws, shift=0, num_heads=nH, head_dim=32,
                         image_layout=False, scale=32 ** -0.5)
    out_w = Fn.WindowAttentionFn.apply(meta_w, qkv_win, bias.detach(), mask_d, None)
    assert_close(out_w, core, dtype, "xl attn out (windows)")
    if mask is not None:  # dense mask, image layout, forward + backward
        q2 = qkv_img.detach().clone().requires_grad_(True)
        b2 = bias.detach().clone().requires_grad_(True)
        out_d = Fn.WindowAttentionFn.apply(meta, q2, b2, mask_d, None)
        assert_close(out_d, ref, dtype, "xl attn out (dense mask)")
        out_d.backward(g)
        assert_close(q2.grad, q64.grad, dtype, "xl dqkv (dense mask)")
        assert_close(b2.grad, b64.grad, dtype, "xl dbias (dense mask)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ws", [13, 15])
def test_xl_attention_padding(ws, dtype):
    """the form of test_wide_attention_padding: every score large and positive (q = k > 0, bias +15), so a padded key that entered the
    softmax would move the row sums; dbias and dqkv are written into poisoned buffers straight through the new entry points"""
    from mtlora_amd import _lib as L
    B, H, W, nH, shift = 2, 2 * ws, ws, 2, ws // 2
    C, N = nH * 32, ws * ws
    torch.manual_seed(ws)
    from mtlora_amd import functional as Fn
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
    assert_close(out, ref, dtype, "xl attn out (padding)")
    assert_close(qkv.grad, q64.grad, dtype, "xl dqkv (padding)")
    assert_close(bias.grad, b64.grad, dtype, "xl dbias (padding)")
    d = meta.desc(dtype)
    lib = L.lib()
    sb = lib.mtlora_window_attn_xl_bwd_scratch_bytes(ctypes.byref(d))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev())
    poison = -12345.678
    dbias = torch.full((nH, N, N), poison, device=dev())
    dqkv = torch.full_like(qkv.detach(), 777.0)
    qc, bc, gc = qkv.detach().contiguous(), bias.detach().contiguous(), g.contiguous()
    st = lib.mtlora_window_attn_xl_bwd(ctypes.byref(d), L.ptr(qc), L.ptr(bc), None, L.ptr(ids), L.ptr(gc), L.ptr(dqkv),
                                       L.ptr(dbias), L.ptr(scratch), sb, L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    assert int((dbias == poison).sum()) == 0 and bool(torch.isfinite(dbias).all())
    assert torch.equal(dbias, bias.grad)
    assert torch.equal(dqkv, qkv.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_xl_attention_backward_is_deterministic(dtype):
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = 4, 28, 42, 3, 14, 7
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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shift, trained", [(7, False), (0, False), (7, True)])
def test_window14_block_vs_oracle(shift, trained, dtype):
    """as test_window12_block_vs_oracle.  trained: the bias comes from a table of trained magnitude (|entries| of order 1, not the
    0.02 of the initialiser) through the gather kernel, and the table's gradient (the scatter kernel) is bit-equal across two runs"""
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerBlock
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    blk = SwinTransformerBlock(64, (28, 28), 2, window_size=14, shift_size=shift, lora=False, tasks=None, mtlora=mt, layer_idx=0)
    O.det_fill_(blk.named_parameters())
    table = blk.attn.relative_position_bias_table
    if trained:
        with torch.no_grad():
            table.copy_(O.det_tensor("w14.table", table.shape, 1.0))
    blk = blk.to(dev()).eval()
    x = O.det_tensor(f"w14.{shift}.x", (2, 28 * 28, 64), 1.0).to(dev()).float().requires_grad_(True)
    gy = None
    tgrads = []
    for _ in range(2 if trained else 1):
        blk.zero_grad(set_to_none=True)
        x.grad = None
        ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
        with ctx:
            y = blk(x)[0]
        gy = O.det_tensor(f"w14.{shift}.gy", y.shape, 1.0) if gy is None else gy
        (y.float() * gy.to(dev())).sum().backward()
        tgrads.append(blk.attn.relative_position_bias_table.grad.clone())
    assert torch.equal(tgrads[0], tgrads[-1])
    ref, x64, P = _oracle_block(blk, x, 14, shift, 2, 28, 28)
    assert_close(y, ref, dtype, "w14 y")
    (ref * gy.double()).sum().backward()
    assert_close(x.grad, x64.grad, dtype, "w14 dx")
    for n, p in blk.named_parameters():
        if not p.requires_grad:  # (frozen pretrained weights)
            continue
        assert p.grad is not None and P["b." + n].grad is not None, n
        assert_close(p.grad, P["b." + n].grad, dtype, f"w14 grad {n}")


def test_xl_attention_dropout_is_refused():
    from mtlora_amd import functional as Fn
    qkv = torch.zeros(1, 14, 14, 96, device=dev())
    bias = torch.zeros(1, 196, 196, device=dev())
    with pytest.raises(RuntimeError, match="144 tokens"):
        Fn.WindowAttentionFn.apply(_meta(1, 14, 14, 1, 14, 0), qkv, bias, None, None, 0.1, 1)
