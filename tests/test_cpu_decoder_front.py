"""Decoder front end, the parts that need no GPU: the portable definition against the literal module sequence, its layout, and the
statuses the entries return before any launch."""
import ctypes

import pytest
import torch

ERR_DTYPE, ERR_SHAPE, ERR_NULL, ERR_UNSUPPORTED = -1, -2, -4, -7  # include/mtlora_hip.h
GRIDS, CS_IN, CS_OUT = [(12, 8), (6, 4), (3, 2), (3, 2)], [32, 64, 96, 96], [18, 36, 72, 144]


def test_portable_definition_is_the_module_sequence():
    """decoder_front_torch == Conv2d(k = 1, bias=False) on the NCHW view -> F.interpolate -> torch.cat in fp64, forward and
    gradients, in the layout of ConcatUpsampleFn.layout with zero pad columns"""
    from mtlora_amd import functional as Fn
    torch.manual_seed(0)
    B, (H, W) = 2, GRIDS[0]
    convs = [torch.nn.Conv2d(C, c, 1, bias=False).double() for C, c in zip(CS_IN, CS_OUT)]
    xs = [torch.randn(B, h * w, C, dtype=torch.float64, requires_grad=True) for (h, w), C in zip(GRIDS, CS_IN)]
    maps = [conv(x.transpose(1, 2).reshape(B, -1, h, w)) for conv, x, (h, w) in zip(convs, xs, GRIDS)]
    ref = torch.cat([maps[0]] + [torch.nn.functional.interpolate(m, (H, W), mode="bilinear") for m in maps[1:]], 1)
    ref = ref.permute(0, 2, 3, 1).reshape(B * H * W, -1)
    got = Fn.decoder_front_torch(xs, [c.weight for c in convs], GRIDS)
    offs, ld = Fn.ConcatUpsampleFn.layout(CS_OUT)
    cols = torch.cat([torch.arange(o, o + c) for o, c in zip(offs, CS_OUT)])
    pad = torch.ones(ld, dtype=torch.bool)
    pad[cols] = False
    assert got.shape == (B * H * W, ld) and (offs, ld) == ([0, 20, 56, 128], 272) and (got[:, pad] == 0).all()
    torch.testing.assert_close(got[:, cols], ref, rtol=1e-12, atol=1e-12)
    gy = torch.randn_like(ref)
    leaves = xs + [c.weight for c in convs]
    for a, b in zip(torch.autograd.grad(got[:, cols], leaves, gy), torch.autograd.grad(ref, leaves, gy)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def _desc(grids=GRIDS, Cs=CS_IN, cs=CS_OUT, dtype=torch.bfloat16, code=None, **over):
    from mtlora_amd import functional as Fn
    d = Fn.decoder_front_desc(2, grids, Cs, cs, dtype)
    d.dtype = d.dtype if code is None else code
    for k, v in over.items():
        setattr(d, k, v)
    return d


CALLS = {"null-desc": (lambda: None, ERR_NULL), "bad-dtype": (lambda: _desc(code=7), ERR_DTYPE),
         "fp32": (lambda: _desc(dtype=torch.float32), ERR_UNSUPPORTED), "one-stage": (lambda: _desc(n=1), ERR_SHAPE),
         "five-stages": (lambda: _desc(n=5), ERR_UNSUPPORTED), "C24": (lambda: _desc(Cs=[24, 64, 96, 96]), ERR_UNSUPPORTED),
         "c38": (lambda: _desc(cs=[18, 38, 72, 144]), ERR_UNSUPPORTED), "c192": (lambda: _desc(cs=[18, 36, 72, 192]), ERR_UNSUPPORTED),
         "scale3": (lambda: _desc(grids=[(12, 6), (4, 2), (4, 2), (4, 2)]), ERR_UNSUPPORTED), "ld": (lambda: _desc(ld=280), ERR_UNSUPPORTED),
         "H-mismatch": (lambda: _desc(h=(ctypes.c_int32 * 4)(12, 6, 3, 4)), ERR_SHAPE),
         "lds": (lambda: _desc(grids=[(8, 4096), (4, 2048), (2, 1024), (2, 1024)]), ERR_UNSUPPORTED), "flags": (lambda: _desc(grad_flags=4), ERR_SHAPE)}


@pytest.mark.parametrize("name", list(CALLS))
def test_entries_refuse_before_any_launch(name):
    """every entry answers the documented status for a descriptor with one defect (the size query -1, the support query 0) without
    touching a pointer"""
    from mtlora_amd import _lib
    make, status = CALLS[name]
    lib, d = _lib.lib(), make()
    d = None if d is None else ctypes.byref(d)
    assert lib.mtlora_decoder_front_supported(d) == 0 and lib.mtlora_decoder_front_bwd_scratch_bytes(d) == -1
    assert lib.mtlora_decoder_front_fwd(d, None, None, None, None) == status
    assert lib.mtlora_decoder_front_bwd(d, None, None, None, None, None, None, 0, None) == status


def test_accepted_descriptor_null_pointers_and_ok():
    from mtlora_amd import _lib
    from mtlora_amd import functional as Fn
    lib, d = _lib.lib(), _desc(grad_flags=3)
    assert lib.mtlora_decoder_front_supported(ctypes.byref(d)) == 1 and lib.mtlora_decoder_front_bwd_scratch_bytes(ctypes.byref(d)) > 0
    assert lib.mtlora_decoder_front_fwd(ctypes.byref(d), None, None, None, None) == ERR_NULL
    assert lib.mtlora_decoder_front_bwd(ctypes.byref(d), None, None, None, None, None, None, 0, None) == ERR_NULL
    assert Fn.decoder_front_desc(2, [(12, 8), (5, 4)], [32, 64], [8, 8], torch.bfloat16) is None      # no integer scale
    assert Fn.decoder_front_desc(2, [(12, 8), (6, 2)], [32, 64], [8, 8], torch.bfloat16) is None      # unequal x / y scales
    assert Fn.decoder_front_desc(2, [(12, 8)] * 5, [32] * 5, [8] * 5, torch.bfloat16) is None         # more than 4 stages
    convs = [torch.nn.Conv2d(C, c, 1, bias=False) for C, c in zip(CS_IN, CS_OUT)]
    xs = [torch.randn(2, h * w, C).bfloat16() for (h, w), C in zip(GRIDS, CS_IN)]
    assert not Fn.decoder_front_ok(xs, convs, GRIDS)  # tensors off the GPU: the caller keeps the separate steps
