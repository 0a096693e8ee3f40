"""MTLORA.BIAS 'all' on the HIP path, host side (no GPU): the library exports ``mtlora_linear_bias_grad``, the ctypes
mirror of ``mtlora_block_grads`` follows the header, and the harness can select the bias mode."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtlora_linear_bias_grad_scratch_bytes", "mtlora_linear_bias_grad")


@pytest.fixture(scope="module")
def built_lib():
    from mtlora_amd.csrc.build import build
    return build(verbose=False)


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtlora_hip.h")).read(), flags=re.S)


def test_library_exports_bias_grad(built_lib):
    """the two entries are additive: library, header and binding agree on the ABI number, which ten existing tests pin at 12 (a
    library from before this change lacks the symbols, so the binding refuses it when it loads)"""
    from mtlora_amd import _lib
    L = _lib.lib()
    m = re.search(r"#define\s+MTLORA_ABI_VERSION\s+(\d+)", header())
    assert m and L.mtlora_version() == _lib.ABI_VERSION == int(m.group(1)) >= 12
    nm = subprocess.run(["nm", "-D", built_lib], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
        assert f" T {name}" in nm, name


def test_ctypes_signatures_of_bias_grad():
    from mtlora_amd import _lib
    P, v = ctypes.POINTER, ctypes.c_void_p
    assert _lib._SIGS[NEW[0]] == (ctypes.c_int64, [P(_lib.LinearDesc)])
    res, args = _lib._SIGS[NEW[1]]
    assert res is ctypes.c_int
    assert args == [P(_lib.LinearDesc), v, P(v), v, v, ctypes.c_int64, v]
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", header()))
    for name in NEW:
        assert protos[name].count(",") + 1 == len(_lib._SIGS[name][1]), name


def test_scratch_query_follows_the_shape_rules(built_lib):
    """N a multiple of the 16-byte vector of the dtype and <= 2^20, M >= 0, T within the task limit; no GPU is touched"""
    from mtlora_amd import _lib
    L = _lib.lib()
    q = lambda d: L.mtlora_linear_bias_grad_scratch_bytes(ctypes.byref(d))
    d = _lib.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T = 197, 96, 96, _lib.BF16, 2
    assert q(d) >= 96 * 4
    d.M = 0
    assert q(d) >= 96 * 4
    d.N = 12  # 1.5 bf16 vectors
    assert q(d) == -1
    d.dtype = _lib.F32  # 3 fp32 vectors
    assert q(d) >= 12 * 4
    d.N, d.dtype = 96, _lib.F16
    assert q(d) >= 96 * 4
    d.dtype = _lib.U8
    assert q(d) == -1
    d.dtype, d.T = _lib.BF16, _lib.MAX_TASKS + 1
    assert q(d) == -1
    d.T, d.N = 0, (1 << 20) + 8
    assert q(d) == -1
    d.N, d.M = 96, -1
    assert q(d) == -1


def test_block_grads_mirror_matches_the_header():
    """same field order, and the size the header implies: every member of mtlora_block_grads is a pointer or an array of pointers"""
    from mtlora_amd import _lib
    body = re.search(r"typedef struct mtlora_block_grads \{(.*?)\} mtlora_block_grads;", header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert re.match(r"^(void|float)\s*\*", decl), decl
        for item in decl.split(","):
            m = re.search(r"\*?\s*([A-Za-z_0-9]+)\s*(?:\[(\d+)\])?\s*$", item.strip())
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert fields[-1] == ("dlin_bias", 4)
    mirror = [(n, ctypes.sizeof(t) // ctypes.sizeof(ctypes.c_void_p)) for n, t in _lib.BlockGrads._fields_]
    assert mirror == fields
    assert ctypes.sizeof(_lib.BlockGrads) == sum(n for _, n in fields) * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.BlockGrads.dlin_bias.offset == _lib.BlockGrads.dbias.offset + ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("bias", ["none", "all"])
def test_build_model_selects_the_bias_mode(bias):
    from mtlora_amd import mtl_harness as H
    model = H.build_model(img_size=56, tasks=("semseg", "normals"), depths=(2, 2), num_heads=(3, 6), r_shared=8, r_task=4, bias=bias)
    named = dict(model.backbone.named_parameters())
    biases = [n for n in named if n.endswith("linear.bias")]
    assert len(biases) == 16  # qkv, proj, fc1, fc2 of four blocks
    assert all(named[n].requires_grad == (bias == "all") for n in biases)
    assert not any(p.requires_grad for n, p in named.items() if n.endswith("linear.weight"))
    assert all(p.requires_grad for n, p in named.items() if "lora_" in n)


def test_build_config_model_passes_the_bias_mode():
    from mtlora_amd import mtl_harness as H
    name = next(iter(H.CONFIGS))
    model = H.build_config_model(name, bias="all", img_size=56, depths=(2, 2), num_heads=(3, 6), embed_dim=96)
    named = dict(model.backbone.named_parameters())
    assert all(p.requires_grad for n, p in named.items() if n.endswith("linear.bias"))
    assert not any(p.requires_grad for n, p in named.items() if n.endswith("linear.weight"))
