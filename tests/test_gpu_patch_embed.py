"""Patch embedding on the HIP path (csrc/patch_embed.hip): gather + GEMM + LayerNorm in one launch each way, held to
``functional.patch_embed_torch`` in fp64 on operands rounded to the compute dtype, at the project's tolerances (x1, relative to
max |ref|)."""
import pytest
import torch

from test_gpu_kernels import TOL, assert_close, dev

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (B, H, W, E): 4 tokens, one partial block, one channel tile | 60 tokens per image, H != W, blocks straddle patch rows and the image
# boundary, ragged last block | the widest accumulators, M = 264: three super blocks of 128 tokens, the last ragged | E = 64: two of
# the three instantiated channel tiles (the skipped-tile paths), M = 315
SHAPES = [(1, 8, 8, 32), (2, 40, 24, 96), (3, 32, 44, 192), (5, 36, 28, 64)]
NAMES = ("weight", "bias", "gamma", "beta")


def _inputs(shape, norm, img_dtype=torch.float32, seed=0):
    B, H, W, E = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    P = {"weight": r(E, 3, 4, 4) * 0.2, "bias": r(E) * 0.5}
    if norm:
        P.update(gamma=1.0 + 0.3 * r(E), beta=0.2 * r(E))
    return r(B, 3, H, W).to(img_dtype), P, r(B, (H // 4) * (W // 4), E)


def _reference(img, P, gy, dtype):
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    from mtlora_amd import functional as Fn
    y = Fn.patch_embed_torch(img.double(), Pd["weight"], Pd["bias"], Pd.get("gamma"), Pd.get("beta"), 1e-5, dtype, torch.float64)
    y.backward(gy.double())
    return y.detach(), {k: v.grad for k, v in Pd.items()}


def _run(img, P, gy, dtype, out_dtype, max_groups=0, train=NAMES):
    from mtlora_amd import functional as Fn
    Pg = {k: v.to(dev()).requires_grad_(k in train) for k, v in P.items()}
    y = Fn.PatchEmbedFn.apply(img.to(dev()), Pg["weight"], Pg["bias"], Pg.get("gamma"), Pg.get("beta"), 1e-5, dtype, out_dtype, max_groups)
    y.backward(gy.to(dev(), out_dtype))
    return y.detach(), {k: v.grad for k, v in Pg.items()}


def _check(shape, dtype, norm, what, out_dtype=torch.float32, img_dtype=torch.float32, max_groups=0):
    img, P, gy = _inputs(shape, norm, img_dtype)
    gy = gy.to(out_dtype).float()  # the gradient as the kernel reads it
    y_ref, g_ref = _reference(img, P, gy, dtype)
    y, grads = _run(img, P, gy, dtype, out_dtype, max_groups)
    assert y.dtype == out_dtype and y.shape == y_ref.shape
    # y in a 16-bit dtype carries that dtype's final rounding (2^-9 / 2^-11 relative, inside the same table)
    assert_close(y, y_ref, dtype, f"patch_embed {what} y")
    for k in P:
        assert_close(grads[k], g_ref[k], dtype, f"patch_embed {what} d{k}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_parity(dtype, norm, shape):
    _check(shape, dtype, norm, f"{dtype} norm={norm} {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_one_workgroup_walks_every_block(dtype, norm, shape):
    """max_groups = 1 on shapes of three super blocks (128 tokens each, the last ragged): one workgroup runs the persistent loop
    three times -- the accumulators carried across iterations, the reuse of the X^T image in LDS, and the forward's loop"""
    assert -(-shape[0] * (shape[1] // 4) * (shape[2] // 4) // 128) == 3
    _check(shape, dtype, norm, f"{dtype} norm={norm} {shape} persist", max_groups=1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=["bf16", "fp16"])
def test_16bit_image_and_output(dtype):
    _check(SHAPES[1], dtype, True, f"{dtype} 16-bit image", out_dtype=dtype, img_dtype=dtype)


@pytest.mark.gpu
def test_gradient_flags_and_reproducibility():
    """With dW / db off, weight.grad and bias.grad are None and dgamma / dbeta are unchanged bit for bit, and the other way
    round; two calls with the same inputs give bit-equal outputs and gradients."""
    img, P, gy = _inputs(SHAPES[1], True)
    y0, g0 = _run(img, P, gy, torch.bfloat16, torch.float32)
    y1, g1 = _run(img, P, gy, torch.bfloat16, torch.float32)
    assert torch.equal(y0, y1) and all(torch.equal(g0[k], g1[k]) for k in NAMES)
    for train in (NAMES[:2], NAMES[2:]):
        y, g = _run(img, P, gy, torch.bfloat16, torch.float32, train=train)
        assert torch.equal(y, y0)
        for k in NAMES:
            assert (g[k] is None) if k not in train else torch.equal(g[k], g0[k]), k


def _count_fused_calls(monkeypatch):
    """calls of functional.patch_embed (the fused route of PatchEmbed.forward) from here on, as a one-element list"""
    from mtlora_amd import functional as Fn
    calls, real = [0], Fn.patch_embed

    def spy(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(Fn, "patch_embed", spy)
    return calls


@pytest.mark.gpu
def test_module_route_matches_the_separate_steps(monkeypatch):
    """PatchEmbed under bf16 autocast with the switch on and off: both held to the fp64 reference, same dtype and shape; the fused
    route is taken exactly when the switch is on and the image wants no gradient."""
    from mtlora_amd import swin_transformer_mtlora as S
    calls = _count_fused_calls(monkeypatch)
    B, H, W, E = SHAPES[1]
    img, P, gy = _inputs(SHAPES[1], True)
    y_ref, g_ref = _reference(img, P, gy, torch.bfloat16)
    mod = S.PatchEmbed(img_size=(H, W), patch_size=4, in_chans=3, embed_dim=E, norm_layer=torch.nn.LayerNorm).to(dev())
    params = {"weight": mod.proj.weight, "bias": mod.proj.bias, "gamma": mod.norm.weight, "beta": mod.norm.bias}
    with torch.no_grad():
        for k, p in params.items():
            p.copy_(P[k])
    prev, outs = S.PATCH_EMBED, []
    try:
        for on in (True, False):
            S.PATCH_EMBED = on
            mod.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = mod(img.to(dev()))
            y.backward(gy.to(dev()))
            outs.append(y)
            assert calls[0] == 1, (on, calls)  # one fused call with the switch on, none more with it off
            assert_close(y, y_ref, torch.bfloat16, f"PatchEmbed switch={on} y")
            for k, p in params.items():
                assert_close(p.grad, g_ref[k], torch.bfloat16, f"PatchEmbed switch={on} d{k}")
        S.PATCH_EMBED = True
        with torch.autocast("cuda", dtype=torch.bfloat16):  # an image that wants a gradient keeps the separate steps, which form one
            x = img.to(dev()).requires_grad_(True)
            mod(x).backward(gy.to(dev()))
        assert calls[0] == 1 and x.grad is not None
    finally:
        S.PATCH_EMBED = prev
    assert outs[0].dtype == outs[1].dtype == torch.float32 and outs[0].shape == outs[1].shape == (B, (H // 4) * (W // 4), E)


@pytest.mark.gpu
def test_fused_route_under_graph_replay(monkeypatch):
    """one train step under GraphedTrainStep with the switch on, the model and the bounds of
    test_gpu_models.test_graphed_train_step_replays_the_eager_step: three replays against three eager steps of the same object --
    losses to 2e-3 relative, the AdamW updates of all trainable parameters pointing the same way (cosine >= 0.98)"""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd import swin_transformer_mtlora as S
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=17, device=dev())
    prev, out, calls = S.PATCH_EMBED, [], _count_fused_calls(monkeypatch)
    S.PATCH_EMBED = True
    try:
        for use_graph in (True, False):
            torch.manual_seed(9)
            Fn._seed_counter = 0
            model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0,
                                  seed=4).to(dev()).train()
            assert model.backbone.patch_embed.proj.weight.requires_grad
            crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, capturable=True)
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2)
            assert gs.graphed, gs.why
            gs.graphed = use_graph
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses = [gs().clone() for _ in range(3)]
            torch.cuda.synchronize()
            out.append((losses, torch.cat([(p.detach() - start[n]).double().flatten() for n, p in model.named_parameters() if n in start])))
    finally:
        S.PATCH_EMBED = prev
        Fn.set_seed_offset(None)
    assert calls[0] >= 2 * 3, calls  # warm-up / capture of both objects and the three eager steps went through the fused route
    for a, b in zip(out[0][0], out[1][0]):
        assert abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (a.item(), b.item())
    cos = (torch.dot(out[0][1], out[1][1]) / (out[0][1].norm() * out[1][1].norm())).item()
    print(f"graph vs eager: losses {[v.item() for v in out[0][0]]} / {[v.item() for v in out[1][0]]}, update cosine {cos:.4f}")
    assert cos >= 0.98, cos
