"""Patch merging on the HIP path (csrc/patch_merge.hip): gather + LayerNorm + reduction in one launch, three backward, held to
``functional.patch_merge_torch`` in fp64 on operands rounded to the compute dtype, at the project's tolerances (x1, relative to
max |ref|)."""
import pytest
import torch

from test_gpu_kernels import assert_close, dev

# (B, H, W, C, n): a single merged row, smallest K | H != W, 30 rows a stream (no multiple of a row block), several streams |
# K = 1536: the weight ring wraps | K = 2048, the limit
SHAPES = [(1, 2, 2, 32, 1), (2, 6, 10, 96, 3), (1, 8, 8, 384, 1), (1, 4, 4, 512, 2)]
NAMES = ("gamma", "beta", "weight")
_ref_cache = {}


def _inputs(shape, dtype, x_dtype):
    """streams with a per-row offset of a few units (a one-pass variance would show), parameters of order 1; everything the kernel
    rounds on the way in (16-bit streams, the weight, the incoming gradient) already rounded"""
    B, H, W, C, n = shape
    g = torch.Generator().manual_seed(sum(shape))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    xs = [(r(B, H * W, C) + 4.0 * r(B, H * W, 1)).to(x_dtype).float() for _ in range(n)]
    P = {"gamma": 1.0 + 0.5 * r(4 * C), "beta": r(4 * C), "weight": r(2 * C, 4 * C).to(dtype).float()}
    return xs, P, r(n * B, H * W // 4, 2 * C).to(dtype).float()


def _reference(shape, dtype, x_dtype):
    key = (shape, dtype, x_dtype)
    if key not in _ref_cache:
        from mtlora_amd import functional as Fn
        xs, P, gy = _inputs(shape, dtype, x_dtype)
        xd = [x.double().requires_grad_(True) for x in xs]
        Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
        y = Fn.patch_merge_torch(xd, Pd["gamma"], Pd["beta"], Pd["weight"], 1e-5, shape[1], shape[2], dtype)
        y.backward(gy.double())
        _ref_cache[key] = (y.detach(), [x.grad for x in xd], {k: v.grad for k, v in Pd.items()})
    return _ref_cache[key]


def _run(shape, dtype, x_dtype, max_groups=0):
    from mtlora_amd import functional as Fn
    xs, P, gy = _inputs(shape, dtype, x_dtype)
    xg = [x.to(dev(), x_dtype).requires_grad_(True) for x in xs]
    Pg = {k: v.to(dev()).requires_grad_(True) for k, v in P.items()}
    y = Fn.PatchMergeFn.apply(Pg["gamma"], Pg["beta"], Pg["weight"], 1e-5, shape[1], shape[2], dtype, max_groups, *xg)
    y.backward(gy.to(dev(), dtype))
    return y.detach(), [x.grad for x in xg], {k: v.grad for k, v in Pg.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("max_groups", [0, 1])
@pytest.mark.parametrize("x32", [True, False], ids=["x-fp32", "x-16bit"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(shape, dtype, x32, max_groups):
    x_dtype = torch.float32 if x32 else dtype
    y_ref, dx_ref, g_ref = _reference(shape, dtype, x_dtype)
    y, dxs, grads = _run(shape, dtype, x_dtype, max_groups)
    what = f"patch_merge {dtype} x32={x32} {shape} groups={max_groups}"
    assert y.dtype == dtype and y.shape == y_ref.shape
    assert_close(y, y_ref, dtype, f"{what} y")
    for k, (dx, ref) in enumerate(zip(dxs, dx_ref)):
        assert dx.dtype == x_dtype
        assert_close(dx, ref, dtype, f"{what} dx{k}")
    for k in NAMES:
        assert grads[k].dtype == torch.float32
        assert_close(grads[k], g_ref[k], dtype, f"{what} d{k}")


@pytest.mark.gpu
def test_bit_reproducible():
    a, b = (_run(SHAPES[1], torch.bfloat16, torch.float32) for _ in range(2))
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    assert all(torch.equal(a[2][k], b[2][k]) for k in NAMES)


@pytest.mark.gpu
def test_module_route_matches_the_separate_steps():
    """PatchMerging(dim=96).forward_multi over three streams under bf16 autocast, switch on against switch off: outputs, stream
    gradients and the three parameters' gradients; same dtype and shape"""
    from types import SimpleNamespace
    from mtlora_amd import swin_transformer_mtlora as S
    B, H, W, C, n = SHAPES[1]
    xs, _, gy = _inputs(SHAPES[1], torch.bfloat16, torch.float32)
    torch.manual_seed(3)
    mod = S.PatchMerging((H, W), dim=C, mtlora=SimpleNamespace(DOWNSAMPLER_ENABLED=False)).to(dev())
    with torch.no_grad():
        mod.norm.weight.add_(0.3 * torch.randn_like(mod.norm.weight))
        mod.norm.bias.add_(0.3 * torch.randn_like(mod.norm.bias))
    params = {"gamma": mod.norm.weight, "beta": mod.norm.bias, "weight": mod.reduction.weight}
    prev, outs = S.PATCH_MERGE, []
    try:
        for on in (False, True):
            S.PATCH_MERGE = on
            mod.zero_grad(set_to_none=True)
            xg = [x.to(dev()).requires_grad_(True) for x in xs]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                assert mod._fused(xg) == on
                ys = mod.forward_multi(xg)
            torch.stack(ys).flatten(0, 1).backward(gy.to(dev(), ys[0].dtype))
            outs.append((torch.stack(ys), [x.grad for x in xg], {k: p.grad.clone() for k, p in params.items()}))
    finally:
        S.PATCH_MERGE = prev
    (y0, dx0, g0), (y1, dx1, g1) = outs
    assert y1.dtype == y0.dtype and y1.shape == y0.shape == (n, B, H * W // 4, 2 * C)
    assert_close(y1, y0, torch.bfloat16, "PatchMerging switch y")
    for k in range(n):
        assert_close(dx1[k], dx0[k], torch.bfloat16, f"PatchMerging switch dx{k}")
    for k in NAMES:
        assert g1[k] is not None
        assert_close(g1[k], g0[k], torch.bfloat16, f"PatchMerging switch d{k}")
