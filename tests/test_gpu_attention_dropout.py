"""Attention dropout inside the fused window attention kernels (csrc/attention_dropout.h): the keep mask element for element
against the oracle's generator, out / dqkv / dbias against an fp64 reference that applies that mask (the project's tolerances,
test_gpu_kernels.TOL, multiplier 1), p = 0, determinism, graph replay with the device seed offset, and the module / model level.

Mask: element (window w, head h, query i, key j) = oracle.dropout_keep_mask_t(seed, STREAM, B_ * nH * N, N, p)[(w * nH + h) * N + i, j]
with w in the order of the reference's (B_, nH, N, N) attention tensor and i, j tokens of the window after the cyclic shift."""
import ctypes

import pytest
import torch

from oracle import mtlora_oracle as O
from test_gpu_kernels import TOL, _regions, assert_close, dev  # noqa: F401  (the suite's helpers and tolerance table)

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5
STREAM = 0x41  # MTL_ATTN_DROP_STREAM
WS = [4, 7, 8, 9, 12]  # N <= 32; one wave, both halves; N = 64 exactly; wide with padded keys; wide at full 144


def _meta(B, H, W, nH, ws, shift, image=True):
    from mtlora_amd import functional as Fn
    return Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=image, scale=SCALE)


def _keep(seed, p, B_, nH, N):
    return O.dropout_keep_mask_t(seed, STREAM, B_ * nH * N, N, p).reshape(B_, nH, N, N)


def _core_drop(qkv, bias, mask, nH, keep, p):
    """oracle.window_attention_core with P' = keep . P / (1 - p) between the softmax and the product with V"""
    B_, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // nH
    q, k, v = qkv.reshape(B_, N, 3, nH, hd).permute(2, 0, 3, 1, 4)
    attn = (q * SCALE) @ k.transpose(-2, -1)
    attn = attn + bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = attn.reshape(B_ // nW, nW, nH, N, N) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.reshape(-1, nH, N, N)
    attn = attn.softmax(-1)
    attn = attn * keep.to(attn.dtype) / (1.0 - p)
    return (attn @ v).transpose(1, 2).reshape(B_, N, C)


def _oracle(qkv_img, bias, mask, nH, ws, shift, H, W, seed, p):
    C, N = nH * 32, ws * ws
    q64 = qkv_img.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True)
    win = O.roll_and_window_partition(q64, shift, ws).reshape(-1, N, 3 * C)
    keep = _keep(seed, p, win.shape[0], nH, N)
    core = _core_drop(win, b64, None if mask is None else mask.double(), nH, keep, p)
    ref = O.window_merge_and_roll(core.reshape(-1, ws, ws, C), shift, ws, H, W)
    return ref, q64, b64, win, core


# ---- 1. the mask, element for element ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", [True, False])
@pytest.mark.parametrize("cfg", [
    # (B, H, W, heads, ws, shift)
    (2, 8, 8, 2, 4, 0), (2, 8, 8, 2, 4, 2), (2, 14, 14, 3, 7, 0), (2, 14, 14, 3, 7, 3), (2, 16, 16, 2, 8, 0), (2, 16, 16, 2, 8, 4),
    (2, 18, 18, 2, 9, 0), (2, 18, 18, 2, 9, 4), (2, 24, 24, 3, 12, 0), (2, 24, 24, 3, 12, 6),
    # more windows than resident workgroups per head: 512 one-wave windows over 256 forward workgroups (8 heads), 128 wide windows
    # over 32, so every workgroup walks its persistent loop and the window index of the mask row moves with it
    (2, 64, 64, 8, 4, 2), (8, 48, 48, 8, 12, 6),
])
def test_mask_element_for_element(cfg, image):
    """q = k = 0 and a zero bias make P uniform (1 / N); with V[j] = e_(j - 32 c) for the 32 keys of chunk c (0 elsewhere),
    out[i][d] * N * (1 - p) is the keep bit of (i, 32 c + d): ceil(N / 32) forwards with one seed read the whole mask back."""
    from mtlora_amd import functional as Fn
    B, H, W, nH, ws, shift = cfg
    p, seed = 0.25, 0x1234_5678_9ABC_DEF1 + ws
    C, N = nH * 32, ws * ws
    B_ = B * (H // ws) * (W // ws)
    if not image:
        shift = 0
    ref = _keep(seed, p, B_, nH, N)
    bias = torch.zeros(nH, N, N, device=dev())
    got = torch.zeros(B_, nH, N, N, dtype=torch.bool)
    for c in range((N + 31) // 32):
        win = torch.zeros(B_, N, 3, nH, 32)
        j = torch.arange(32 * c, min(32 * c + 32, N))
        win[:, j, 2, :, j - 32 * c] = 1.0
        win = win.reshape(B_, N, 3 * C)
        if image:
            qkv = O.window_merge_and_roll(win.reshape(-1, ws, ws, 3 * C), shift, ws, H, W).contiguous().to(dev())
            out = Fn.WindowAttentionFn.apply(_meta(B, H, W, nH, ws, shift), qkv, bias, None, None, p, seed)
            out = O.roll_and_window_partition(out.cpu(), shift, ws).reshape(B_, N, C)
        else:
            meta = _meta(B_, ws, ws, nH, ws, 0, image=False)
            out = Fn.WindowAttentionFn.apply(meta, win.to(dev()), bias, None, None, p, seed).cpu()
        bits = out.reshape(B_, N, nH, 32).permute(0, 2, 1, 3).double() * N * (1.0 - p)  # [w][h][i][d]
        assert bool(((bits - bits.round()).abs() <= 1e-5).all()) and bool(((bits.round() == 0) | (bits.round() == 1)).all())
        got[..., 32 * c:32 * c + 32] = bits.round().bool()[..., :len(j)]
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} keep bits differ"
    assert 0.70 < ref.float().mean().item() < 0.80


# ---- 2. parity with the fp64 reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("ws", WS)
def test_parity_vs_fp64_reference(ws, p, dtype):
    """image layout + region ids (shifted), image layout + dense mask, window layout + dense mask, image layout without a mask
    (unshifted): out, dqkv, dbias"""
    from mtlora_amd import functional as Fn
    B, H, W, nH, shift = 2, 2 * ws, 2 * ws, 3 if ws != 12 else 2, ws // 2
    C, N = nH * 32, ws * ws
    seed = 0xC0FFEE_0000_0001 * ws + int(p * 10)
    torch.manual_seed(ws * 10 + nH)
    qkv0 = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype)
    bias0 = torch.randn(nH, N, N, device=dev()) * 0.5
    mask = O.shifted_window_mask(H, W, ws, shift)
    mask_d, ids = mask.to(dev()), _regions(H, W, ws, shift).to(dev())
    ref, q64, b64, win, core = _oracle(qkv0, bias0, mask, nH, ws, shift, H, W, seed, p)
    g = torch.randn(B, H, W, C, device=dev()).to(dtype)
    ref.backward(g.double().cpu())
    meta = _meta(B, H, W, nH, ws, shift)
    for what, m_arg, i_arg in (("ids", None, ids), ("dense", mask_d, None)):
        q, b = qkv0.clone().requires_grad_(True), bias0.clone().requires_grad_(True)
        out = Fn.WindowAttentionFn.apply(meta, q, b, m_arg, i_arg, p, seed)
        out.backward(g)
        assert_close(out, ref, dtype, f"attn-drop out ({what})")
        assert_close(q.grad, q64.grad, dtype, f"attn-drop dqkv ({what})")
        assert_close(b.grad, b64.grad, dtype, f"attn-drop dbias ({what})")
    # window layout, dense mask
    nW = mask.shape[0]
    qw = win.detach().to(dev()).to(dtype).contiguous().requires_grad_(True)
    bw = bias0.clone().requires_grad_(True)
    meta_w = _meta(qw.shape[0] // nW, ws, ws * nW, nH, ws, 0, image=False)
    out_w = Fn.WindowAttentionFn.apply(meta_w, qw, bw, mask_d, None, p, seed)
    assert_close(out_w, core, dtype, "attn-drop out (windows)")
    gw = O.roll_and_window_partition(g.cpu(), shift, ws).reshape(-1, N, C).to(dev()).contiguous()
    out_w.backward(gw)
    assert_close(qw.grad, O.roll_and_window_partition(q64.grad, shift, ws).reshape(-1, N, 3 * C), dtype, "attn-drop dqkv (windows)")
    assert_close(bw.grad, b64.grad, dtype, "attn-drop dbias (windows)")
    # no mask, unshifted
    ref0, q640, b640, _, _ = _oracle(qkv0, bias0, None, nH, ws, 0, H, W, seed, p)
    ref0.backward(g.double().cpu())
    q, b = qkv0.clone().requires_grad_(True), bias0.clone().requires_grad_(True)
    out = Fn.WindowAttentionFn.apply(_meta(B, H, W, nH, ws, 0), q, b, None, None, p, seed)
    out.backward(g)
    assert_close(out, ref0, dtype, "attn-drop out (no mask)")
    assert_close(q.grad, q640.grad, dtype, "attn-drop dqkv (no mask)")
    assert_close(b.grad, b640.grad, dtype, "attn-drop dbias (no mask)")


# ---- 3. p = 0 -----------------------------------------------------------------------------------------------------------------
def _abi(meta, dtype, qkv, bias, ids, g, drop):
    """forward + backward straight through the C ABI; drop = None: the plain entry points"""
    from mtlora_amd import _lib as L
    lib, d = L.lib(), meta.desc(dtype)
    out, dqkv, dbias = torch.empty_like(g), torch.empty_like(qkv), torch.empty_like(bias)
    sb = lib.mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev())
    if drop is None:
        st = lib.mtlora_window_attn_fwd(ctypes.byref(d), L.ptr(qkv), L.ptr(bias), None, L.ptr(ids), L.ptr(out), L.stream_ptr())
        assert st == 0
        st = lib.mtlora_window_attn_bwd(ctypes.byref(d), L.ptr(qkv), L.ptr(bias), None, L.ptr(ids), L.ptr(g), L.ptr(dqkv), L.ptr(dbias),
                                        L.ptr(scratch), sb, L.stream_ptr())
    else:
        st = lib.mtlora_window_attn_drop_fwd(ctypes.byref(d), ctypes.byref(drop), L.ptr(qkv), L.ptr(bias), None, L.ptr(ids), L.ptr(out),
                                             L.stream_ptr())
        assert st == 0
        st = lib.mtlora_window_attn_drop_bwd(ctypes.byref(d), ctypes.byref(drop), L.ptr(qkv), L.ptr(bias), None, L.ptr(ids), L.ptr(g),
                                             L.ptr(dqkv), L.ptr(dbias), L.ptr(scratch), sb, L.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    return out, dqkv, dbias


def _inputs(ws, dtype, nH=2, B=2):
    H = W = 2 * ws
    shift, C, N = ws // 2, nH * 32, ws * ws
    torch.manual_seed(ws)
    qkv = (torch.randn(B, H, W, 3 * C, device=dev()) * 0.7).to(dtype)
    bias = torch.randn(nH, N, N, device=dev()) * 0.5
    ids = _regions(H, W, ws, shift).to(dev())
    g = torch.randn(B, H, W, C, device=dev()).to(dtype)
    return _meta(B, H, W, nH, ws, shift), qkv, bias, ids, g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ws", [7, 12])
def test_p_zero_is_the_plain_path(ws, dtype):
    from mtlora_amd import _lib as L
    meta, qkv, bias, ids, g = _inputs(ws, dtype)
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = 0.0, 99, None
    for a, b in zip(_abi(meta, dtype, qkv, bias, ids, g, None), _abi(meta, dtype, qkv, bias, ids, g, dr)):
        assert torch.equal(a, b)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ws", [7, 12])
def test_same_seed_same_bits_other_seed_other_mask(ws, dtype):
    from mtlora_amd import _lib as L
    meta, qkv, bias, ids, g = _inputs(ws, dtype)
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = 0.3, 4242, None
    a, b = _abi(meta, dtype, qkv, bias, ids, g, dr), _abi(meta, dtype, qkv, bias, ids, g, dr)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x.float()).all())
    dr.seed = 4243
    c = _abi(meta, dtype, qkv, bias, ids, g, dr)
    assert not torch.equal(a[0], c[0])


# ---- 5. graph replay with the device seed offset ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [7, 12])
def test_graph_replay_draws_the_mask_of_seed_plus_offset(ws):
    from mtlora_amd import functional as Fn
    dtype, p, seed = torch.bfloat16, 0.2, 0xFFFF_FFFF  # (seed + 1 carries into the high word)
    meta, qkv, bias, ids, _ = _inputs(ws, dtype)
    eager = [Fn.WindowAttentionFn.apply(meta, qkv, bias, None, ids, p, seed + k) for k in (0, 1)]
    off = torch.zeros(1, dtype=torch.int64, device=dev())
    Fn.set_seed_offset(off)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            Fn.WindowAttentionFn.apply(meta, qkv, bias, None, ids, p, seed)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = Fn.WindowAttentionFn.apply(meta, qkv, bias, None, ids, p, seed)
        got = []
        for k in (0, 1):
            off.fill_(k)
            graph.replay()
            torch.cuda.synchronize()
            got.append(out.clone())
    finally:
        Fn.set_seed_offset(None)
    assert not torch.equal(eager[0], eager[1])
    for a, b in zip(got, eager):
        assert torch.equal(a, b)


# ---- 6. module and model level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ws", [7, 12])
def test_window_attention_module_with_attn_drop(ws, dtype, monkeypatch):
    """WindowAttention(attn_drop=0.1): in training the fused core (between the qkv and proj linears) matches the fp64 reference
    with the generator's mask, forward and backward; in eval it is bit-equal to the same module without attention dropout"""
    from mtlora_amd import functional as Fn
    from mtlora_amd import swin_transformer_mtlora as S
    nH, p, seed = 2, 0.1, 0x5EED_0000_0000_0007
    C, N = nH * 32, ws * ws
    mt = O.mtlora_config([], r_shared=8, r_task=4, dropout=0.0)
    attn = S.WindowAttention(C, (ws, ws), nH, attn_drop=p, mtlora=mt, layer_idx=0)
    O.det_fill_(attn.named_parameters())
    attn = attn.to(dev()).train()
    monkeypatch.setattr(Fn, "next_seed", lambda: seed)
    held = {}
    dense_bias = attn.dense_bias

    def keep_bias():
        b = dense_bias()
        b.retain_grad()
        held["bias"] = b
        return b

    attn.dense_bias = keep_bias
    h1 = attn.qkv.register_forward_hook(lambda m, a, o: (o[0].retain_grad(), held.__setitem__("qkv", o[0]))[0])
    h2 = attn.proj.register_forward_pre_hook(lambda m, a: (a[0].retain_grad(), held.__setitem__("core", a[0]))[0])
    mask = O.shifted_window_mask(2 * ws, 2 * ws, ws, ws // 2)
    x = O.det_tensor(f"attn_drop.{ws}.x", (2 * mask.shape[0], N, C), 1.0).to(dev()).float()
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        y, _ = attn(x, mask.to(dev()))
    y.float().square().sum().backward()
    h1.remove()
    h2.remove()
    qkv, core, bias = held["qkv"], held["core"], held["bias"]
    q64 = qkv.detach().double().cpu().requires_grad_(True)
    b64 = bias.detach().double().cpu().requires_grad_(True)
    ref = _core_drop(q64, b64, mask.double(), nH, _keep(seed, p, q64.shape[0], nH, N), p)
    ref.backward(core.grad.double().cpu())
    assert_close(core, ref, dtype, "module core")
    assert_close(qkv.grad, q64.grad, dtype, "module dqkv")
    assert_close(bias.grad, b64.grad, dtype, "module dbias")
    assert attn.relative_position_bias_table.grad is not None and bool(torch.isfinite(attn.relative_position_bias_table.grad).all())
    # eval: no dropout, the kernels of a module without it
    del attn.dense_bias
    plain = S.WindowAttention(C, (ws, ws), nH, attn_drop=0.0, mtlora=mt, layer_idx=0).to(dev())
    plain.load_state_dict(attn.state_dict())
    with torch.no_grad(), ctx:
        a, b = attn.eval()(x, mask.to(dev()))[0], plain.eval()(x, mask.to(dev()))[0]
    assert torch.equal(a, b)


def test_model_trains_with_attention_dropout_eagerly_and_replayed():
    """SwinTransformerMTLoRA(attn_drop_rate=0.1) with tasks (four stages of two blocks, the model of
    test_graphed_train_step_replays_the_eager_step: the harness heads' fused concat-upsample trains four-stage backbones only): one
    eager train_step and GraphedTrainStep replays have a finite loss and finite gradients.  With a zero learning rate (and no other dropout) the parameters stand still, so the losses
    of two replays differ through the attention masks alone -- the device seed offset moves them."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd import swin_transformer_mtlora as S
    tasks = ["semseg", "normals"]
    # the constructor argument reaches every attention module (build_model has no such argument: it builds the shipped configs) ...
    mt = H.mtlora_namespace(tasks, 8, 4, n_stages=2, dropout=0.0)
    bb = S.SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                                 window_size=7, attn_drop_rate=0.1, drop_path_rate=0.0, tasks=tasks, mtlora=mt)
    assert [m.attn_drop.p for m in bb.modules() if isinstance(m, S.WindowAttention)] == [0.1] * 4
    # ... which is all it does, so the harness model gets the rate the same way
    model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=8, r_task=4, drop_path_rate=0.0, seed=5, dropout=0.0)
    for m in model.modules():
        if isinstance(m, S.WindowAttention):
            m.attn_drop.p = 0.1
    model = model.to(dev()).train()
    img, tg = H.synthetic_batch(2, 224, tasks, seed=3, device=dev())
    crit = H.MultiTaskLoss(tasks)
    opt = H.build_optimizer(model, lr=0.0, capturable=True)
    calls = [0]
    orig = Fn.WindowAttentionFn.forward

    def counting(ctx, meta, qkv, bias, mask, mask_ids, *drop):
        calls[0] += 1 if drop and drop[0] > 0 else 0
        return orig(ctx, meta, qkv, bias, mask, mask_ids, *drop)

    Fn.WindowAttentionFn.forward = staticmethod(counting)
    try:
        loss, norm = H.train_step(model, crit, opt, img, tg)  # (norm: the total gradient norm before clipping)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(torch.as_tensor(norm)).all()) and float(norm) > 0.0
        assert calls[0] == 8  # every block's attention drew a mask
        gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2)
        assert gs.graphed, gs.why
        losses = [gs().clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in losses)
        assert all(bool(torch.isfinite(q.grad).all()) for q in model.parameters() if q.requires_grad and q.grad is not None)
        assert losses[0].item() != losses[1].item()
    finally:
        Fn.WindowAttentionFn.forward = staticmethod(orig)
        Fn.set_seed_offset(None)
