"""Patch embedding, the parts that need no GPU: the portable definition against the literal module sequence, the C ABI's
symbols, and the statuses the entries return before any launch."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mtlora_patch_embed_supported", "mtlora_patch_embed_fwd", "mtlora_patch_embed_bwd_scratch_bytes", "mtlora_patch_embed_bwd")
ERR_DTYPE, ERR_NULL, ERR_UNSUPPORTED = -1, -4, -7  # include/mtlora_hip.h


@pytest.mark.parametrize("norm", [True, False])
def test_portable_definition_is_the_module_sequence(norm):
    """patch_embed_torch == Conv2d(k = s = 4) -> flatten -> transpose -> LayerNorm in fp64, forward and gradients"""
    from mtlora_amd import functional as Fn
    torch.manual_seed(0)
    conv, ln = torch.nn.Conv2d(3, 32, 4, 4).double(), torch.nn.LayerNorm(32).double()
    with torch.no_grad():
        ln.weight.add_(torch.randn(32).double() * 0.3)
        ln.bias.add_(torch.randn(32).double() * 0.3)
    img, gy = torch.randn(2, 3, 12, 20).double(), torch.randn(2, 15, 32).double()
    ref = conv(img).flatten(2).transpose(1, 2)
    ref = ln(ref) if norm else ref
    params = [conv.weight, conv.bias] + ([ln.weight, ln.bias] if norm else [])
    g_ref = torch.autograd.grad(ref, params, gy)
    got = Fn.patch_embed_torch(img, conv.weight, conv.bias, ln.weight if norm else None, ln.bias if norm else None, ln.eps,
                               torch.float64, torch.float64)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    for a, b in zip(torch.autograd.grad(got, params, gy), g_ref):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def test_symbols_in_header_and_exports():
    from mtlora_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtlora_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    for name in NAMES:
        assert name in protos and name in _lib.EXPORTS and protos[name].count(",") + 1 == len(_lib._SIGS[name][1]), name


def _desc(**over):
    from mtlora_amd import _lib
    d = _lib.PatchEmbedDesc()
    d.B, d.in_chans, d.H, d.W, d.patch, d.E = 2, 3, 8, 8, 4, 96
    d.img_dtype, d.dtype, d.out_dtype, d.has_norm, d.eps, d.grad_flags = _lib.F32, _lib.BF16, _lib.F32, 1, 1e-5, 3
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over, status", [(None, ERR_NULL), ({"dtype": 7}, ERR_DTYPE), ({"patch": 2}, ERR_UNSUPPORTED),
                                          ({"E": 40}, ERR_UNSUPPORTED), ({"H": 6}, ERR_UNSUPPORTED)],
                         ids=["null-desc", "bad-dtype", "patch2", "E40", "H6"])
def test_entries_refuse_before_any_launch(over, status):
    """every entry answers the documented status (the size query -1, the support query 0) without touching a pointer"""
    from mtlora_amd import _lib
    lib = _lib.lib()
    d = None if over is None else ctypes.byref(_desc(**over))
    assert lib.mtlora_patch_embed_supported(d) == 0
    assert lib.mtlora_patch_embed_bwd_scratch_bytes(d) == -1
    assert lib.mtlora_patch_embed_fwd(d, *[None] * 9) == status
    assert lib.mtlora_patch_embed_bwd(d, *[None] * 12, 0, None) == status


def test_accepted_descriptor_and_null_pointers():
    from mtlora_amd import _lib
    lib, d = _lib.lib(), ctypes.byref(_desc())
    assert lib.mtlora_patch_embed_supported(d) == 1 and lib.mtlora_patch_embed_bwd_scratch_bytes(d) > 0
    assert lib.mtlora_patch_embed_fwd(d, *[None] * 9) == ERR_NULL
    assert lib.mtlora_patch_embed_bwd(d, *[None] * 12, 0, None) == ERR_NULL
