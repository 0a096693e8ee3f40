"""Window attention for windows up to 12 x 12: what the entry points decide BEFORE any launch (no GPU needed) -- which window sizes
are accepted, the error a rejected shape gets, and that the scratch sizes of the one-wave (N <= 64) path did not move."""
import ctypes

import pytest

OK, SHAPE, UNSUPPORTED = 0, -2, -7


@pytest.fixture(scope="module")
def L():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    _lib.lib()
    return _lib


def _desc(L, ws, H, W, B=2, heads=3, head_dim=32, shift=0, dtype=None, image_layout=1):
    d = L.AttnDesc()
    d.B, d.H, d.W = B, H, W
    d.window_size, d.shift = ws, shift
    d.num_heads, d.head_dim = heads, head_dim
    d.image_layout = image_layout
    d.dtype = 1 if dtype is None else dtype  # MTLORA_F32 0 / MTLORA_BF16 1 / MTLORA_F16 2
    d.scale = 32 ** -0.5
    d.mask_value = -100.0
    return d


def _fwd(L, d):
    # validation comes first: a rejected descriptor returns before the (null) pointers are looked at
    return L.lib().mtlora_window_attn_fwd(ctypes.byref(d), None, None, None, None, None, None)


def _bwd(L, d):
    return L.lib().mtlora_window_attn_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, 0, None)


def test_window_12_is_validated_not_rejected(L):
    """window_size 12 with a map it does not divide is a SHAPE error (H % ws), as for window 7 -- not 'unsupported'"""
    d = _desc(L, 12, 25, 24)
    assert _fwd(L, d) == SHAPE
    assert _bwd(L, d) == SHAPE
    assert L.lib().mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d)) == -1
    d7 = _desc(L, 7, 15, 14)
    assert _fwd(L, d7) == SHAPE


@pytest.mark.parametrize("ws", [9, 10, 11, 12])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_wide_windows_size_their_scratch(L, ws, dtype):
    d = _desc(L, ws, 2 * ws, 2 * ws, dtype=dtype)
    sb = L.lib().mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d))
    N = ws * ws
    assert sb >= 0
    # at least one (nH, N, N) fp32 partial, never more partials than windows
    assert 3 * N * N * 4 <= sb <= 8 * 3 * N * N * 4 + 256


def test_window_12_on_24x24(L):
    d = _desc(L, 12, 24, 24, shift=6)
    assert L.lib().mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d)) >= 0


@pytest.mark.parametrize("ws", [13, 14, 16])
def test_windows_above_12_stay_unsupported(L, ws):
    d = _desc(L, ws, 2 * ws, 2 * ws)
    assert _fwd(L, d) == UNSUPPORTED
    assert _bwd(L, d) == UNSUPPORTED
    assert L.lib().mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d)) == -1


def test_other_limits_unchanged(L):
    assert _fwd(L, _desc(L, 12, 24, 24, head_dim=64)) == UNSUPPORTED
    assert _fwd(L, _desc(L, 12, 24, 24, shift=12)) == SHAPE
    assert _fwd(L, _desc(L, 12, 24, 24, dtype=7)) == -1  # MTLORA_ERR_DTYPE


def test_narrow_scratch_sizes_unchanged(L):
    """the N <= 64 launch path is not touched.  The constants are mtlora_window_attn_bwd_scratch_bytes of the commit before the
    multi-wave kernels (G partials of (nH, N, N) fp32 + 256, G = min(windows, 256 * resident workgroups per CU / heads))."""
    parent = {
        # (B, H, W, heads, ws, dtype): bytes
        (2, 16, 16, 2, 8, 1): 262400,        # 8 windows: one partial per window
        (2, 16, 16, 2, 8, 0): 262400,
        (64, 56, 56, 3, 7, 1): 9825148,      # 341 groups
        (64, 56, 56, 3, 7, 0): 4898296,      # 170 groups (fp32 images: two workgroups per CU)
        (64, 64, 64, 4, 8, 1): 16777472,     # 256 groups
        (64, 64, 64, 4, 8, 2): 16777472,
        (64, 64, 64, 4, 8, 0): 8388864,      # 128 groups
    }
    for (B, H, W, nH, ws, dt), want in parent.items():
        d = _desc(L, ws, H, W, B=B, heads=nH, dtype=dt)
        assert L.lib().mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d)) == want, (B, H, W, nH, ws, dt)


def test_abi_version_and_exports_unchanged(L):
    assert L.ABI_VERSION == 12 and L.lib().mtlora_version() == 12


def test_wide_kernels_use_no_scratch(tmp_path):
    """a condition of the multi-wave kernels, not a measurement: every instantiation of k_attn_wide_fwd / _bwd compiles to 0 bytes of
    scratch per lane (the backward lives on the whole register file of a SIMD; a spill there is a silent slowdown).  Read from the
    compiler's resource remarks of the device pass of attention.hip (no GPU needed, ~30 s)."""
    import os
    import re
    import subprocess
    from mtlora_amd.csrc import build as B
    src = os.path.join(B.HERE, "attention.hip")
    p = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                                 str(tmp_path / "attention.dev.o")], capture_output=True, text=True, cwd=B.HERE)
    assert p.returncode == 0, p.stderr[-2000:]
    scratch, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur is not None:
            scratch[cur] = int(m.group(1))
    wide = {k: v for k, v in scratch.items() if "k_attn_wide_" in k}
    assert len(wide) == 12, sorted(wide)  # forward and backward x fp32 / bf16 / fp16 x dense mask or not
    assert all(v == 0 for v in wide.values()), {k: v for k, v in wide.items() if v}
