"""Window attention for 13 x 13 to 16 x 16 windows (144 < N <= 256, csrc/attention_xl.h): what the new entry points decide BEFORE
any launch, and the CSR lists of the bias scatter (no GPU needed)."""
import ctypes

import pytest
import torch

from test_cpu_attention_wide import SHAPE, UNSUPPORTED, L, _desc  # noqa: F401  (the library fixture and the descriptor helper)


def _fwd(L, d):
    return L.lib().mtlora_window_attn_xl_fwd(ctypes.byref(d), None, None, None, None, None, None)


def _bwd(L, d):
    return L.lib().mtlora_window_attn_xl_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, 0, None)


def test_xl_exports_are_additive(L):
    names = {"mtlora_window_attn_xl_fwd", "mtlora_window_attn_xl_bwd", "mtlora_window_attn_xl_bwd_scratch_bytes",
             "mtlora_rel_bias_gather", "mtlora_rel_bias_scatter"}
    assert names <= set(L.EXPORTS) and all(hasattr(L.lib(), n) for n in names)
    assert L.ABI_VERSION == 12 and L.lib().mtlora_version() == 12


@pytest.mark.parametrize("d_kw, want", [
    (dict(ws=14, H=29, W=28), SHAPE), (dict(ws=16, H=32, W=40), SHAPE),
    (dict(ws=12, H=24, W=24), UNSUPPORTED), (dict(ws=17, H=34, W=34), UNSUPPORTED), (dict(ws=14, H=28, W=28, head_dim=64), UNSUPPORTED),
    (dict(ws=14, H=28, W=28, dtype=7), -1), (dict(ws=14, H=28, W=28, shift=14), SHAPE),
])
def test_xl_validation(L, d_kw, want):
    d = _desc(L, **d_kw)
    assert _fwd(L, d) == want
    assert _bwd(L, d) == want
    assert L.lib().mtlora_window_attn_xl_bwd_scratch_bytes(ctypes.byref(d)) == -1


@pytest.mark.parametrize("ws", [13, 14, 15, 16])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_xl_windows_size_their_scratch(L, ws, dtype):
    d = _desc(L, ws, 2 * ws, 2 * ws, dtype=dtype, shift=ws // 2)
    sb = L.lib().mtlora_window_attn_xl_bwd_scratch_bytes(ctypes.byref(d))
    N, heads, windows = ws * ws, 3, 2 * 4
    # at least one (nH, N, N) fp32 partial plus 3 N floats of row statistics per (window, head); never more partials than windows
    stats = windows * heads * 3 * N * 4
    assert heads * N * N * 4 + stats <= sb <= windows * heads * N * N * 4 + stats + 256
    assert _fwd(L, d) == -4 and _bwd(L, d) == -4  # validated: the null pointers are what is wrong now (MTLORA_ERR_NULL)


def test_rel_bias_csr_covers_every_position_once():
    from mtlora_amd import functional as Fn
    from mtlora_amd.swin_transformer_mtlora import _relative_position_index
    index = _relative_position_index(14, 14)
    off, pos = Fn.rel_bias_csr(index, 27 * 27)
    assert off.dtype == pos.dtype == torch.int32 and off.shape == (27 * 27 + 1,) and int(off[0]) == 0 and int(off[-1]) == 196 * 196
    assert torch.equal(torch.sort(pos.long()).values, torch.arange(196 * 196))
    flat = index.reshape(-1)
    for e in (0, 1, 364, 728):  # corners and the centre (the diagonal: all 196 positions i == j)
        seg = pos[int(off[e]):int(off[e + 1])].long()
        assert bool((flat[seg] == e).all()) and bool((seg[1:] > seg[:-1]).all()) and len(seg) == int((flat == e).sum())
    with pytest.raises(RuntimeError):
        Fn.rel_bias_csr(index, 27 * 27 - 1)
