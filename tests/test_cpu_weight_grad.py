"""Full fine-tuning on the HIP path, host side (no GPU): the library exports ``mtlora_linear_weight_grad`` (+ its size query) and
``mtlora_linear_weight_cast``, the ctypes tables follow the header, the ABI number stays 12, and the portable definition
``functional.weight_grad_torch`` is autograd's ``linear.weight.grad`` of the oracle's MTLoRALinear (fp64, 1e-12 max-norm relative)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from oracle import mtlora_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtlora_linear_weight_grad_scratch_bytes", "mtlora_linear_weight_grad", "mtlora_linear_weight_cast")


@pytest.fixture(scope="module")
def built_lib():
    from mtlora_amd.csrc.build import build
    return build(verbose=False)


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtlora_hip.h")).read(), flags=re.S)


def test_header_declares_the_three_exports():
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", header()))
    for name in NEW:
        assert name in protos, name
    assert re.search(r"int64_t\s+mtlora_linear_weight_grad_scratch_bytes\s*\(\s*const mtlora_linear_desc\s*\*", header())
    assert "float* dW" in protos["mtlora_linear_weight_grad"] and "const void* const* dy_t" in protos["mtlora_linear_weight_grad"]
    assert protos["mtlora_linear_weight_cast"].startswith("const float* W")


def test_library_exports_them_and_the_abi_stays_12(built_lib):
    from mtlora_amd import _lib
    L = _lib.lib()
    m = re.search(r"#define\s+MTLORA_ABI_VERSION\s+(\d+)", header())
    assert m and L.mtlora_version() == _lib.ABI_VERSION == int(m.group(1)) == 12
    nm = subprocess.run(["nm", "-D", built_lib], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
        assert f" T {name}" in nm, name


def test_ctypes_signatures_match_the_prototypes():
    from mtlora_amd import _lib
    P, v, i = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGS[NEW[0]] == (ctypes.c_int64, [P(_lib.LinearDesc)])
    assert _lib._SIGS[NEW[1]] == (i, [P(_lib.LinearDesc), v, v, P(v), v, v, ctypes.c_int64, v])
    assert _lib._SIGS[NEW[2]] == (i, [v, i, i, i, v, v, v])
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", header()))
    for name in NEW:
        assert protos[name].count(",") + 1 == len(_lib._SIGS[name][1]), name


def test_size_query_follows_the_shape_rules(built_lib):
    """N and K multiples of the 16-byte vector of the dtype, M >= 0, T within the task limit; no GPU is touched"""
    from mtlora_amd import _lib
    L = _lib.lib()
    q = lambda d: L.mtlora_linear_weight_grad_scratch_bytes(ctypes.byref(d))
    d = _lib.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T = 197, 96, 288, _lib.BF16, 2
    assert q(d) > 0
    d.M = 0
    assert q(d) > 0
    d.N = 12  # 1.5 bf16 vectors
    assert q(d) == -1
    d.dtype = _lib.F32  # 3 fp32 vectors
    assert q(d) > 0
    d.N, d.K, d.dtype = 288, 20, _lib.F16  # K off the grid
    assert q(d) == -1
    d.K, d.dtype = 96, _lib.U8
    assert q(d) == -1
    d.dtype, d.T = _lib.BF16, _lib.MAX_TASKS + 1
    assert q(d) == -1
    d.T, d.M = 0, -1
    assert q(d) == -1
    # a long reduction over a small output is split over M: the partial tiles need room
    d.M, d.N, d.K = 401408, 288, 96
    assert q(d) >= 2 * 3 * 128 * 128 * 4


def test_entry_rejects_before_any_launch(built_lib):
    """the argument checks need no device: NULL pointers and a refused shape come back as error codes"""
    from mtlora_amd import _lib
    L = _lib.lib()
    d = _lib.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T = 16, 96, 288, _lib.BF16, 0
    null, none = ctypes.c_void_p(0), _lib.ptr_array(None)
    assert L.mtlora_linear_weight_grad(ctypes.byref(d), null, null, none, null, null, 0, null) == -4  # MTLORA_ERR_NULL
    d.N = 12
    assert L.mtlora_linear_weight_grad(ctypes.byref(d), null, null, none, null, null, 0, null) == -2  # MTLORA_ERR_SHAPE
    assert L.mtlora_linear_weight_cast(null, 8, 8, _lib.BF16, null, null, null) == -4
    assert L.mtlora_linear_weight_cast(null, 0, 8, _lib.BF16, null, null, null) == -2


TASKS = ["a", "b"]
CASES = {
    "no_tasks": dict(T=0),
    "two_tasks_shared_input": dict(T=2),
    "two_tasks_x_tasks": dict(T=2, x_tasks=True),
    "one_output_gradient_missing": dict(T=2, x_tasks=True, drop=1),
    "shared_gradient_missing": dict(T=2, drop=0),
    "matrixv2": dict(T=2, x_tasks=True, shared_mode="matrixv2"),
    "matrixv2_shared_input": dict(T=2, shared_mode="matrixv2"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_weight_grad_torch_is_autograds_linear_weight_grad(case):
    """(3, 7) leading shape, K = 24, N = 40, r 8 / 4 / 4: the portable definition against autograd through the oracle's MTLoRALinear"""
    from mtlora_amd import functional as Fn
    c = CASES[case]
    tasks = TASKS[:c["T"]]
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    K, N = 24, 40
    x = rnd(3, 7, K)
    xt = {t: rnd(3, 7, K) for t in tasks} if c.get("x_tasks") else None
    W, b = rnd(N, K).requires_grad_(True), rnd(N)
    A_s, B_s = rnd(8, K), rnd(N, 8)
    A_t, B_t = {t: rnd(4, K) for t in tasks}, {t: rnd(N, 4) for t in tasks}
    y, yt = O.mtlora_linear(x, W, b, A_s, B_s, 2.0, tasks=tasks or None, A_t=A_t, B_t=B_t, scale_t={t: 1.5 for t in tasks}, x_tasks=xt,
                            shared_mode=c.get("shared_mode", "matrix"))
    outs = [y] + [yt[t] for t in tasks]
    dys = [rnd(3, 7, N) for _ in outs]
    if "drop" in c:
        dys[c["drop"]] = None
    torch.autograd.backward([o for o, d in zip(outs, dys) if d is not None], [d for d in dys if d is not None])
    got = Fn.weight_grad_torch(x, dys)
    assert got.shape == (N, K) and got.dtype == torch.float64
    err = ((got - W.grad).abs().max() / W.grad.abs().max()).item()
    assert err <= 1e-12, err


def test_weight_grad_torch_needs_a_gradient():
    from mtlora_amd import functional as Fn
    with pytest.raises(ValueError):
        Fn.weight_grad_torch(torch.zeros(4, 8), [None, None])


def test_build_model_unfrozen_trains_every_linear_weight():
    from mtlora_amd import mtl_harness as H
    model = H.build_model(img_size=56, tasks=("semseg", "normals"), depths=(2, 2), num_heads=(3, 6), r_shared=8, r_task=4, freeze=False)
    named = dict(model.backbone.named_parameters())
    weights = [n for n in named if n.endswith("linear.weight")]
    assert len(weights) == 16 and all(named[n].requires_grad for n in weights)
    assert "FREEZE_PRETRAINED" in H.build_model.__doc__
