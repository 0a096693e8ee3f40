"""Rank-aware dense update, host side: exports, the portable definitions, the untouched ATen fallback and the argument rejects."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32, (8,)), (96, 40, (33,)), (40, 96, (100, 8, 33))]
NAMES = ("mtlora_delta_fwd", "mtlora_delta_bwd")


@pytest.fixture(scope="module")
def lib():
    from mtlora_amd import _lib
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    return _lib.lib()


def test_symbols_and_abi(lib):
    from mtlora_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtlora_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    nm = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert name in _lib.EXPORTS and f" T {name}" in nm and protos[name].count(",") + 1 == len(_lib._SIGS[name][1]), name
    assert "const float* const* Z, float* const* dA, float* const* dB, void* stream" in " ".join(protos["mtlora_delta_bwd"].split())
    assert lib.mtlora_version() == _lib.ABI_VERSION == 12 and "#define MTLORA_ABI_VERSION 12" in hdr


def _inputs(N, K, rs):
    g = torch.Generator().manual_seed(N * 1000 + K)
    mk = lambda *s: torch.randn(*s, generator=g)
    return [mk(r, K) for r in rs], [mk(N, r) for r in rs], [mk(N, K) for _ in rs]


@pytest.mark.parametrize("N,K,rs", SHAPES)
def test_portable_definitions_against_fp64(N, K, rs):
    from mtlora_amd import functional as Fn
    As, Bs, Zs = _inputs(N, K, rs)
    sc, sd = [0.5 * (i + 1) for i in range(len(rs))], [torch.tensor([-1.5])] + [None] * (len(rs) - 1)
    dW = Fn.delta_torch(As, Bs, sc, sd)
    dA, dB = Fn.delta_bwd_torch(As, Bs, sc, Zs, sd)
    for i, (a, b, z) in enumerate(zip(As, Bs, Zs)):
        a, b, z, s = a.double(), b.double(), z.double(), sc[i] * (-1.5 if i == 0 else 1.0)
        for got, ref, mag, n_red in ((dW[i], b @ a, b.abs() @ a.abs(), rs[i]), (dA[i], b.t() @ z, b.abs().t() @ z.abs(), N),
                                     (dB[i], z @ a.t(), z.abs() @ a.abs().t(), K)):
            assert bool(((got.double() - s * ref).abs() <= (n_red + 4) * 2.0 ** -24 * abs(s) * mag).all())


@pytest.mark.parametrize("rs", [(128, 128), (128, 100), (256,)])
def test_fallback_on_cpu_tensors_is_unchanged(rs):
    """CPU factors do not qualify for the HIP path: _delta_factors returns the bits of the ATen sequence it always ran"""
    from mtlora_amd import lora
    As, Bs, _ = _inputs(288, 96, rs)
    sc = [2.0, 1.5][:len(rs)]
    eyes, dW = lora._delta_factors(As, Bs, sc, 96, 288)
    if len(rs) > 1 and len(set(rs)) == 1:
        want = list((torch.bmm(torch.stack(Bs), torch.stack(As)) * torch.tensor(sc).view(-1, 1, 1)).unbind(0))
    else:
        want = [(b @ a) * s for a, b, s in zip(As, Bs, sc)]
    assert all(torch.equal(g, w) for g, w in zip(dW, want)) and all(torch.equal(e, torch.eye(96)) for e in eyes)


@pytest.mark.parametrize("defect,code", [("n0", -2), ("K6", -2), ("r0", -2), ("null_elem", -4), ("misaligned_A", -3)])
@pytest.mark.parametrize("fn", NAMES)
def test_rejects_leave_outputs_untouched(lib, fn, defect, code):
    from mtlora_amd import _lib as L
    N, K, rs = 40, 8, [5, 3]
    As, Bs, Zs = _inputs(N, K, rs)
    outs = [[torch.full((N, K), 7.0) for _ in rs]] if fn == NAMES[0] else [Zs] + [[torch.full_like(t, 7.0) for t in ts] for ts in (As, Bs)]
    n, K = 0 if defect == "n0" else 2, 6 if defect == "K6" else K
    if defect == "r0":
        rs[1] = 0
    elif defect == "null_elem":
        Bs[1] = None
    elif defect == "misaligned_A":
        As[0] = torch.zeros(5 * 8 + 1)[1:]
    st = getattr(lib, fn)(n, N, K, (ctypes.c_int32 * 2)(*rs), L.ptr_array9(As), L.ptr_array9(Bs), (ctypes.c_float * 2)(1.0, 1.0), None,
                          *[L.ptr_array9(o) for o in outs], None)
    assert st == code
    assert all(bool((t == 7.0).all()) for ts in outs[-2:] for t in ts if ts is not Zs)
