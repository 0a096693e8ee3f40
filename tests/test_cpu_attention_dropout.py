"""Attention dropout entry points, host side (no GPU): the two exports, every rejection before a launch, and the compiler's scratch
figure of every new kernel."""
import ctypes
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def L():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    return _lib


def _desc(L, ws=7, head_dim=32, nH=3):
    d = L.AttnDesc()
    d.B, d.H, d.W, d.window_size, d.shift = 2, 2 * ws, 2 * ws, ws, 0
    d.num_heads, d.head_dim, d.image_layout, d.dtype = nH, head_dim, 1, L.BF16
    d.scale, d.mask_value = head_dim ** -0.5, -100.0
    return d


def _drop(L, p):
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = p, 1234, None
    return dr


def _calls(L, d, dr):
    """status of the forward and the backward entry point.  The data pointers are fake (16-byte aligned, never dereferenced by the
    host): a call that got past validation would have to launch, which without a device cannot return one of the statuses below."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    drp = None if dr is None else ctypes.byref(dr)
    f = lib.mtlora_window_attn_drop_fwd(ctypes.byref(d), drp, fake, fake, None, None, fake, None)
    b = lib.mtlora_window_attn_drop_bwd(ctypes.byref(d), drp, fake, fake, None, None, fake, fake, fake, fake, 1 << 40, None)
    return f, b


def test_symbols_exported(L):
    assert {"mtlora_window_attn_drop_fwd", "mtlora_window_attn_drop_bwd"} <= set(L.EXPORTS)
    nm = subprocess.run(["nm", "-D", L.LIB_PATH], capture_output=True, text=True).stdout
    for s in ("mtlora_window_attn_drop_fwd", "mtlora_window_attn_drop_bwd"):
        assert f" T {s}" in nm, s
    assert ctypes.sizeof(L.AttnDropout) == 24 and L.AttnDropout.seed.offset == 8 and L.AttnDropout.seed_offset.offset == 16


ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = -4, -2, -7


def test_status_codes_are_the_headers(L):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtlora_hip.h")).read()
    for name, val in (("MTLORA_ERR_NULL", ERR_NULL), ("MTLORA_ERR_SHAPE", ERR_SHAPE), ("MTLORA_ERR_UNSUPPORTED", ERR_UNSUPPORTED)):
        m = re.search(name + r"\s*=?\s*(-?\d+)", hdr)
        assert m and int(m.group(1)) == val, name


@pytest.mark.parametrize("p", [1.0, 1.5, -0.1, float("nan"), float("inf")])
def test_bad_probability_is_a_shape_error(L, p):
    assert _calls(L, _desc(L), _drop(L, p)) == (ERR_SHAPE, ERR_SHAPE)


def test_null_dropout_struct(L):
    assert _calls(L, _desc(L), None) == (ERR_NULL, ERR_NULL)


def test_null_data_pointers_after_a_valid_dropout(L):
    d, dr = _desc(L), _drop(L, 0.1)
    lib = L.lib()
    assert lib.mtlora_window_attn_drop_fwd(ctypes.byref(d), ctypes.byref(dr), None, None, None, None, None, None) == ERR_NULL
    assert lib.mtlora_window_attn_drop_bwd(ctypes.byref(d), ctypes.byref(dr), None, None, None, None, None, None, None, None, 0,
                                           None) == ERR_NULL


@pytest.mark.parametrize("ws", [13, 16])
def test_windows_13_to_16_stay_unsupported(L, ws):
    assert _calls(L, _desc(L, ws=ws), _drop(L, 0.1)) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)


def test_head_dim_64_is_unsupported(L):
    assert _calls(L, _desc(L, head_dim=64), _drop(L, 0.1)) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)


def test_mask_rows_must_fit_32_bits(L):
    """n_windows * nH * N >= 2^32 cannot index the generator (the plain entry points accept the shape)"""
    d = _desc(L, ws=8, nH=32)
    d.B = 1 << 22  # 2^22 images x 4 windows x 32 heads x 64 tokens = 2^35 rows
    assert _calls(L, d, _drop(L, 0.1)) == (ERR_SHAPE, ERR_SHAPE)


def test_new_kernels_use_no_scratch(L, tmp_path):
    """every attention-dropout kernel (k_attn_drop_fwd / _bwd, k_attn_drop_wide_fwd / _bwd: 4 x fp32 / bf16 / fp16 x dense mask or
    not = 24) reports 0 bytes of scratch per lane in the compiler's resource remarks, read as test_wide_kernels_use_no_scratch reads
    them.  (The wide backward keeps its register dbias accumulator; the one-wave kernels launder the lane id per window and query
    half, and the fp32 one-wave backward loads a window's rows in its own iteration: DESIGN 5b.)"""
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
    new = {k: v for k, v in scratch.items() if "k_attn_drop_" in k}
    print(sorted(new.items()))
    assert len(new) == 24, sorted(new)
    wide = {k: v for k, v in new.items() if "k_attn_drop_wide_" in k}
    assert len(wide) == 12 and all(v == 0 for v in wide.values()), {k: v for k, v in wide.items() if v}
    assert all(v == 0 for v in new.values()), {k: v for k, v in new.items() if v}
