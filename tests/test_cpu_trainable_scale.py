"""Device-resident (trainable) LoRA scales, host side (no GPU): the additive exports and their bindings, every rejection of the new
entries before a launch, the descriptor left alone, and the portable scale-gradient definition against autograd."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtlora_linear_pack_dev", "mtlora_linear_pack_entry_dev", "mtlora_linear_scale_grad", "mtlora_linear_scale_grad_scratch_bytes")


@pytest.fixture(scope="module")
def L():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def codes():
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    out = {}
    for name in ("MTLORA_OK", "MTLORA_ERR_SHAPE", "MTLORA_ERR_ALIGN", "MTLORA_ERR_NULL", "MTLORA_ERR_WORKSPACE"):
        m = re.search(name + r"\s*=\s*(-?\d+)", hdr)
        assert m, name
        out[name[len("MTLORA_"):]] = int(m.group(1))
    assert out["OK"] == 0 and len(set(out.values())) == 5
    return out


def test_entries_declared_exported_and_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtlora_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    nm = subprocess.run(["nm", "-D", L.LIB_PATH], capture_output=True, text=True).stdout
    lib = L.lib()
    for name in NEW:
        assert name in protos and name in L.EXPORTS and hasattr(lib, name), name
        assert f" T {name}" in nm, name
        res, args = L._SIGS[name]
        params = protos[name].strip()
        assert len(args) == (0 if params in ("", "void") else params.count(",") + 1), name
    # the *_dev forms are the by-value forms plus (scale_dev, n_scale) in front of the destination
    for name in ("mtlora_linear_pack", "mtlora_linear_pack_entry"):
        old, new = L._SIGS[name][1], L._SIGS[name + "_dev"][1]
        assert new == old[:5] + [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int] + old[5:], name
        assert "const float* const* scale_dev, int n_scale" in protos[name + "_dev"]
        assert protos[name + "_dev"].replace("const float* const* scale_dev, int n_scale, ", "").split() == protos[name].split()
    assert L._SIGS["mtlora_linear_scale_grad_scratch_bytes"][0] is ctypes.c_int64
    assert lib.mtlora_version() == L.ABI_VERSION == 12
    assert re.search(r"#define\s+MTLORA_ABI_VERSION\s+12\b", hdr)


def _desc(L, T=3, rs=8):
    d = L.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T, d.r_s = 1, 96, 288, L.BF16, T, rs
    for i in range(T):
        d.r_t[i] = 4
        d.scale_t[i] = 1.0
    d.scale_s = 1.0
    return d


def _arr(vals):
    a = (ctypes.c_void_p * 9)()
    for i, v in enumerate(vals):
        a[i] = v
    return a


def test_descriptor_is_unchanged(L):
    """the scale pointers travel as arguments: mtlora_linear_desc keeps its fields"""
    assert [f[0] for f in L.LinearDesc._fields_] == ["M", "K", "N", "dtype", "mode", "T", "r_s", "r_t", "scale_s", "scale_t", "has_x_tasks",
                                                     "dropout_p", "seed", "seed_offset", "bwd_phase", "sel_stream", "sel_dense", "sel_tn",
                                                     "sel_projk", "max_cu", "packed", "hid", "hid_pad_", "hid_ptr"]


@pytest.mark.parametrize("entry", ["mtlora_linear_pack_dev", "mtlora_linear_pack_entry_dev"])
def test_pack_dev_rejections(L, codes, entry):
    """null destinations, a wrong pointer count, misaligned scale pointers: the documented codes, before any launch (the fake
    addresses below are never dereferenced on the host, and nothing is launched)"""
    lib = L.lib()
    d = _desc(L)
    need = lib.mtlora_linear_packed_bytes(ctypes.byref(d))
    assert need > 0
    A = ctypes.c_void_p(0x1000)
    At, Bt = _arr([0x2000, 0x3000, 0x4000]), _arr([0x5000, 0x6000, 0x7000])
    sc = _arr([0x5A5A5100, 0, 0x5A5A5108, 0x5A5A510C])  # (a null slot is legal: that segment is a constant)
    host = (ctypes.c_ubyte * lib.mtlora_linear_pack_entry_bytes())()
    last = ctypes.byref(host) if entry.endswith("entry_dev") else None
    fn = getattr(lib, entry)
    call = lambda scale, n, dst, nbytes=need, tail=last: fn(ctypes.byref(d), A, A, At, Bt, scale, n, dst, nbytes, tail)
    dst = ctypes.c_void_p(0x10000)
    assert call(sc, 4, None) == codes["ERR_NULL"]                      # null destination
    assert call(sc, 4, ctypes.c_void_p(0x10004)) == codes["ERR_ALIGN"]  # destination off 16 bytes
    assert call(sc, 4, dst, need - 512) == codes["ERR_WORKSPACE"]
    assert call(None, 4, dst) == codes["ERR_NULL"]                     # null scale array
    for n in (0, 1, 3, 5, 9):
        assert call(sc, n, dst) == codes["ERR_SHAPE"], n               # count != 1 + T
    for bad in (0x101, 0x102, 0x10A):
        assert call(_arr([0x100, bad, 0, 0]), 4, dst) == codes["ERR_ALIGN"], bad
        assert call(_arr([bad, 0, 0, 0]), 4, dst) == codes["ERR_ALIGN"], bad
    if entry.endswith("entry_dev"):
        assert call(sc, 4, dst, need, None) == codes["ERR_NULL"]       # null host entry
        assert call(sc, 4, dst) == codes["OK"]                         # a pure host call: fills the record
        assert (0x5A5A510C).to_bytes(8, "little") in bytes(host)            # (the record holds the scales' addresses)
        assert call(_arr([0, 0, 0, 0]), 4, dst) == codes["OK"]         # all constant: what the by-value entry writes
        assert (0x5A5A510C).to_bytes(8, "little") not in bytes(host)
    d.K = 100  # an invalid descriptor is rejected first, as by the by-value entries
    want = lib.mtlora_linear_pack_entry(ctypes.byref(d), A, A, At, Bt, dst, need, ctypes.byref(host))
    assert want != codes["OK"] and call(sc, 4, dst) == want and call(sc, 5, dst) == want


def test_scale_grad_rejections(L, codes):
    lib = L.lib()
    d = _desc(L)
    sb = lib.mtlora_linear_scale_grad_scratch_bytes()
    assert sb >= 9 * 4
    dB, B = _arr([0x1000, 0x2000, 0x3000, 0x4000]), _arr([0x5000, 0x6000, 0x7000, 0x8000])
    sc = _arr([0x100, 0x104, 0, 0x10C])
    out, scr = ctypes.c_void_p(0x200), ctypes.c_void_p(0x10000)
    call = lambda dB_=dB, B_=B, sc_=sc, n=4, o=out, s=scr, nb=sb: lib.mtlora_linear_scale_grad(ctypes.byref(d), dB_, B_, sc_, n, o, s, nb, None)
    assert call(o=None) == codes["ERR_NULL"]
    assert call(s=None) == codes["ERR_NULL"]
    assert call(dB_=None) == codes["ERR_NULL"] and call(B_=None) == codes["ERR_NULL"] and call(sc_=None) == codes["ERR_NULL"]
    for n in (0, 3, 5):
        assert call(n=n) == codes["ERR_SHAPE"], n
    assert call(sc_=_arr([0x100, 0x106, 0, 0])) == codes["ERR_ALIGN"]
    assert call(o=ctypes.c_void_p(0x202)) == codes["ERR_ALIGN"]
    assert call(dB_=_arr([0x1001, 0, 0, 0])) == codes["ERR_ALIGN"]
    assert call(nb=sb - 4) == codes["ERR_WORKSPACE"]
    assert call(B_=_arr([0, 0x6000, 0x7000, 0x8000])) == codes["ERR_NULL"]  # a live segment without its master
    # nothing to form (every segment lacks its scale or its dB): OK without a launch
    assert call(dB_=_arr([0, 0, 0x3000, 0]), sc_=_arr([0x100, 0x104, 0, 0x10C])) == codes["OK"]


def test_linear_meta_carries_scale_tensors_and_fills_ones():
    from mtlora_amd import functional as Fn
    s0, s2 = torch.tensor([2.5]), torch.tensor([0.7])
    meta = Fn.LinearMeta(K=96, N=288, r_s=8, r_t=(4, 4), scale_s=s0, scale_t=(3.0, s2), mode=0, has_x_tasks=True, dropout_p=0.0, seed=0,
                         dtype=torch.float32)
    sd = meta.scale_dev
    assert sd[0] is s0 and sd[1] is None and sd[2] is s2
    d = meta.desc(1)
    assert d.scale_s == 1.0 and d.scale_t[0] == 3.0 and d.scale_t[1] == 1.0
    meta = Fn.LinearMeta(K=96, N=288, r_s=8, r_t=(4,), scale_s=2.0, scale_t=(3.0,), mode=0, has_x_tasks=True, dropout_p=0.0, seed=0,
                         dtype=torch.float32)
    assert meta.scale_dev is None


def test_forward_has_no_item_on_the_scales():
    """the forward path of MTLoRALinear reads no scale on the host"""
    import inspect
    from mtlora_amd.lora import MTLoRALinear
    src = inspect.getsource(MTLoRALinear.forward)
    assert ".item()" not in src and ".cpu()" not in src and "float(s.detach()" not in src


@pytest.mark.parametrize("mode", ["shared", "task_xt", "dropout"])
def test_scale_grad_torch_against_autograd_fp64(mode):
    """y = s * (x_in A^T) B^T: autograd's d loss / d s against <dB, B> / s formed from autograd's dB"""
    from mtlora_amd import functional as Fn
    torch.manual_seed(3)
    Mr, K, N, r = 37, 24, 40, 5
    x = torch.randn(Mr, K, dtype=torch.float64)
    if mode == "dropout":
        x = x * (torch.rand(Mr, K) > 0.3) / 0.7
    A = torch.randn(r, K, dtype=torch.float64, requires_grad=True)
    B = torch.randn(N, r, dtype=torch.float64, requires_grad=True)
    s = torch.tensor([1.7 if mode == "shared" else -0.45], dtype=torch.float64, requires_grad=True)
    W = torch.randn(N, K, dtype=torch.float64)
    y = x @ W.t() + (x @ A.t() @ B.t()) * s
    (y * torch.randn(Mr, N, dtype=torch.float64)).sum().backward()
    got = Fn.scale_grad_torch(B.grad, B.detach(), s.detach())
    assert got.shape == (1,) and got.dtype == torch.float32
    torch.testing.assert_close(got.double(), s.grad, rtol=1e-6, atol=0.0)
    got32 = Fn.scale_grad_torch(B.grad.float(), B.detach().float(), s.detach().float())
    torch.testing.assert_close(got32.double(), s.grad, rtol=1e-5, atol=0.0)
    assert Fn.scale_grad_torch(B.grad, B.detach(), torch.zeros(1)).item() == 0.0
