"""Patch merging, the parts that need no GPU: the C ABI's symbols, the statuses the entries return before any launch, the portable
definition against the literal module sequence, and the module's route on CPU tensors."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mtlora_patch_merge_fwd", "mtlora_patch_merge_bwd", "mtlora_patch_merge_bwd_scratch_bytes")
ERR_NULL, ERR_UNSUPPORTED = -4, -7  # include/mtlora_hip.h


def test_symbols_in_header_exports_and_library():
    from mtlora_amd import _lib
    text = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    for name in NAMES:
        assert name in protos and name in _lib.EXPORTS and protos[name].count(",") + 1 == len(_lib._SIGS[name][1]), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 12 and re.search(r"#define\s+MTLORA_ABI_VERSION\s+12\b", text) and _lib.lib().mtlora_version() == 12


def _desc(**over):
    from mtlora_amd import _lib
    d = _lib.PatchMergeDesc()
    d.B, d.n, d.H, d.W, d.C, d.x_dtype, d.dtype, d.eps = 2, 3, 6, 10, 96, _lib.F32, _lib.BF16, 1e-5
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _call_all(d):
    from mtlora_amd import _lib
    lib = _lib.lib()
    return (lib.mtlora_patch_merge_fwd(d, *[None] * 8), lib.mtlora_patch_merge_bwd(d, *[None] * 12, 0, None),
            lib.mtlora_patch_merge_bwd_scratch_bytes(d))


@pytest.mark.parametrize("over, status", [(None, ERR_NULL), ({}, ERR_NULL), ({"C": 48}, ERR_UNSUPPORTED), ({"C": 544}, ERR_UNSUPPORTED),
                                          ({"H": 7}, ERR_UNSUPPORTED), ({"dtype": 0}, ERR_UNSUPPORTED), ({"B": 0}, 0)],
                         ids=["null-desc", "null-pointers", "C48", "C544", "odd-H", "fp32", "zero-rows"])
def test_entries_answer_before_any_launch(over, status):
    fwd, bwd, size = _call_all(None if over is None else ctypes.byref(_desc(**over)))
    assert fwd == status and bwd == status
    assert size == -1 if over is None or status == ERR_UNSUPPORTED else size >= 0


def test_scratch_query_positive_and_monotone_in_rows():
    from mtlora_amd import _lib
    sizes = [_lib.lib().mtlora_patch_merge_bwd_scratch_bytes(ctypes.byref(_desc(B=b))) for b in (1, 2, 8, 64, 512, 4096)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]


def test_portable_definition_is_the_module_sequence():
    """patch_merge_torch in fp64 == explicit gather -> nn.LayerNorm(4C) -> nn.Linear(4C, 2C, bias=False): outputs and all gradients,
    two streams, H != W"""
    from mtlora_amd import functional as Fn
    torch.manual_seed(0)
    B, H, W, C = 2, 4, 6, 8
    ln, lin = torch.nn.LayerNorm(4 * C).double(), torch.nn.Linear(4 * C, 2 * C, bias=False).double()
    with torch.no_grad():
        ln.weight.add_(torch.randn(4 * C).double() * 0.3)
        ln.bias.add_(torch.randn(4 * C).double() * 0.3)
    xs = [torch.randn(B, H * W, C).double().requires_grad_(True) for _ in range(2)]
    gy = torch.randn(2 * B, H * W // 4, 2 * C).double()

    def gather(x):  # the reference's cat order (swin_transformer_mtlora.py PatchMerging.forward)
        x = x.view(B, H, W, C)
        return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).view(B, -1, 4 * C)
    ref = torch.cat([lin(ln(gather(x))) for x in xs])
    params = [ln.weight, ln.bias, lin.weight]
    g_ref = torch.autograd.grad(ref, xs + params, gy)
    got = Fn.patch_merge_torch(xs, ln.weight, ln.bias, lin.weight, ln.eps, H, W, torch.bfloat16)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    for a, b in zip(torch.autograd.grad(got, xs + params, gy), g_ref):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def test_module_keeps_the_separate_steps_on_cpu(monkeypatch):
    from mtlora_amd import functional as Fn
    from mtlora_amd import swin_transformer_mtlora as S
    monkeypatch.setattr(S, "PATCH_MERGE", True)
    monkeypatch.setattr(Fn, "patch_merge", lambda *a, **k: pytest.fail("fused route taken on CPU tensors"))
    mod = S.PatchMerging((4, 6), dim=32, mtlora=SimpleNamespace(DOWNSAMPLER_ENABLED=False))
    xs = [torch.randn(2, 24, 32) for _ in range(2)]
    ys = mod.forward_multi(xs)
    assert len(ys) == 2 and ys[0].shape == (2, 6, 64)
    torch.testing.assert_close(ys[1], mod(xs[1]))
