"""Activation dropout entry points, host side (no GPU): the four exports and their bindings, the portable definitions against the
oracle's generator, every rejection before a launch, and the compiler's scratch figure of every new kernel."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from oracle import mtlora_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtlora_act_dropout_fwd", "mtlora_act_dropout_bwd", "mtlora_residual_droppath_drop_fwd", "mtlora_residual_droppath_drop_bwd")
SITES = {"HIDDEN": 0x42, "PROJ": 0x43, "MLP_OUT": 0x44, "POS": 0x45}


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
    for name in ("MTLORA_OK", "MTLORA_ERR_DTYPE", "MTLORA_ERR_SHAPE", "MTLORA_ERR_ALIGN", "MTLORA_ERR_NULL"):
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
        assert res is ctypes.c_int and len(args) == protos[name].count(",") + 1, name
        assert "const mtlora_attn_dropout* drop" in protos[name] and ctypes.POINTER(L.AttnDropout) in args
    assert lib.mtlora_version() == L.ABI_VERSION == 12
    assert re.search(r"#define\s+MTLORA_ABI_VERSION\s+12\b", hdr)


def test_stream_ids_are_the_headers(L):
    from mtlora_amd import functional as Fn
    common = open(os.path.join(ROOT, "mtlora_amd", "csrc", "common.h")).read()
    for name, val in SITES.items():
        m = re.search(r"MTL_ACT_DROP_" + name + r"\s*=\s*(0x[0-9A-Fa-f]+)u", common)
        assert m and int(m.group(1), 16) == val == getattr(L, "ACT_DROP_" + name), name
    m = re.search(r"MTL_ACT_DROP_TENSOR_STRIDE\s*=\s*(0x[0-9A-Fa-f]+)u", common)
    assert m and int(m.group(1), 16) == 0x100 == L.ACT_DROP_TENSOR_STRIDE
    for site in SITES.values():
        for k in range(9):
            assert Fn.act_dropout_stream(site, k) == site + 0x100 * k
    ids = [Fn.act_dropout_stream(s, k) for s in SITES.values() for k in range(9)]
    assert len(set(ids)) == 36 and 0 not in ids and 0x41 not in ids  # (the linear layers' and the attention kernels' streams)


SEED, ROWS, COLS = 0x1234_5678_9ABC_DEF1, 37, 24


def test_keep_mask_is_the_oracles_and_differs_per_tensor_and_site(L):
    from mtlora_amd import functional as Fn
    masks = {}
    for site in SITES.values():
        for k in range(9):
            m = Fn.act_dropout_keep(SEED, site, k, ROWS, COLS, 0.3)
            assert torch.equal(m, O.dropout_keep_mask(SEED, site + 0x100 * k, ROWS, COLS, 0.3)), (site, k)
            masks[(site, k)] = m
    keys = list(masks)
    for i, a in enumerate(keys):
        assert 0.5 < masks[a].float().mean().item() < 0.9
        for b in keys[i + 1:]:
            assert not torch.equal(masks[a], masks[b]), (a, b)
    assert Fn.act_dropout_keep(SEED, 0x42, 0, ROWS, COLS, 0.0).all()
    assert Fn.act_dropout_keep(SEED, 0x42, 0, ROWS, COLS, 2.0 ** -17).all()  # below 2^-16: off


@pytest.mark.parametrize("act", [0, 1])
def test_act_dropout_torch_on_the_cpu(L, act):
    from mtlora_amd import functional as Fn
    torch.manual_seed(0)
    p, site = 0.25, 0x42
    hs = [torch.randn(ROWS, COLS) for _ in range(3)]
    out = Fn.act_dropout_torch(hs, act, p, SEED, site)
    for k, (h, o) in enumerate(zip(hs, out)):
        keep = O.dropout_keep_mask(SEED, site + 0x100 * k, ROWS, COLS, p)
        ref = torch.where(keep, (torch.nn.functional.gelu(h) if act else h) / (1 - p), torch.zeros(()))
        torch.testing.assert_close(o, ref, rtol=1e-6, atol=1e-7)
        assert (o[~keep] == 0).all()


@pytest.mark.parametrize("shared", [True, False])
def test_residual_droppath_drop_torch_on_the_cpu(L, shared):
    from mtlora_amd import functional as Fn
    torch.manual_seed(1)
    p, site, n, B, T, C = 0.5, 0x43, 3, 2, 5, 16
    res = torch.randn(B, T, C) if shared else [torch.randn(B, T, C) for _ in range(n)]
    ys = [torch.randn(B, T, C) for _ in range(n)]
    scale = (torch.rand(n, B) < 0.7).float() / 0.7
    out = Fn.residual_droppath_drop_torch(res, ys, scale, p, SEED, site)
    for k in range(n):
        keep = O.dropout_keep_mask(SEED, site + 0x100 * k, B * T, C, p).view(B, T, C)
        r = res if shared else res[k]
        ref = r + scale[k].view(B, 1, 1) * torch.where(keep, ys[k] / (1 - p), torch.zeros(()))
        torch.testing.assert_close(out[k], ref, rtol=1e-6, atol=1e-7)
        assert torch.equal(out[k][~keep], r[~keep])


# ---- host rejections: one defect per call.  The data pointers are fake (aligned, never dereferenced by the host): a call that got
# past validation would have to launch, which without a device cannot return one of the statuses below
def _args(L, **kw):
    a = dict(n=2, M=64, C=16, B=2, dtype=L.BF16, rdt=L.F32, ydt=L.BF16, p=0.1, act=1, drop=True, ptr=0x1000, bad_k=None, bad_ptr=0,
             arrays=True)
    a.update(kw)
    return a


def _arr(L, a, n):
    if not a["arrays"]:
        return None
    arr = L.PtrArr9()
    for k in range(n):
        arr[k] = a["ptr"]
    if a["bad_k"] is not None:
        arr[a["bad_k"]] = a["bad_ptr"]
    return arr


def _call(L, entry, **kw):
    a = _args(L, **kw)
    lib = L.lib()
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = a["p"], 99, None
    drp = ctypes.byref(dr) if a["drop"] else None
    n = a["n"]
    good = L.PtrArr9()
    for k in range(min(max(n, 0), 9)):
        good[k] = 0x1000
    bad = _arr(L, a, min(max(n, 0), 9))
    if entry == "mtlora_act_dropout_fwd":
        return lib.mtlora_act_dropout_fwd(n, bad, good, drp, 0x42, a["act"], a["M"], a["C"], a["dtype"], None)
    if entry == "mtlora_act_dropout_bwd":
        return lib.mtlora_act_dropout_bwd(n, bad, good, good, drp, 0x42, a["act"], a["M"], a["C"], a["dtype"], None)
    if entry == "mtlora_residual_droppath_drop_fwd":
        return lib.mtlora_residual_droppath_drop_fwd(n, good, bad, good, None, drp, 0x43, a["M"], a["C"], a["B"], a["rdt"], a["ydt"], None)
    return lib.mtlora_residual_droppath_drop_bwd(n, bad, good, None, None, drp, 0x43, a["M"], a["C"], a["B"], a["rdt"], a["ydt"], None)


@pytest.mark.parametrize("entry", NEW)
def test_host_rejections(L, codes, entry):
    res = "residual" in entry
    assert _call(L, entry, dtype=7, rdt=7) == codes["ERR_DTYPE"]
    if res:
        assert _call(L, entry, rdt=L.F16, ydt=L.BF16) == codes["ERR_DTYPE"]  # no bf16 <-> fp16 mix
    for n in (0, 10, -1):
        assert _call(L, entry, n=n) == codes["ERR_SHAPE"], n
    assert _call(L, entry, drop=False) == codes["ERR_NULL"]
    assert _call(L, entry, arrays=False) == codes["ERR_NULL"]
    if entry != "mtlora_residual_droppath_drop_bwd":  # (its g / dy elements may be NULL, as the plain entry's)
        assert _call(L, entry, bad_k=1, bad_ptr=0) == codes["ERR_NULL"]
    assert _call(L, entry, bad_k=1, bad_ptr=0x1008) == codes["ERR_ALIGN"]
    for C in (12, 4, 0):
        assert _call(L, entry, C=C) == codes["ERR_SHAPE"], C
    if res:
        assert _call(L, entry, M=63, B=2) == codes["ERR_SHAPE"]
        assert _call(L, entry, B=0) == codes["ERR_SHAPE"]
    else:
        assert _call(L, entry, act=2) == codes["ERR_SHAPE"]
    for p in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert _call(L, entry, p=p) == codes["ERR_SHAPE"], p
    assert _call(L, entry, M=1 << 32, B=1) == codes["ERR_SHAPE"]
    # nothing to do: OK without a launch (a launch could not succeed here)
    assert _call(L, entry, M=0) == codes["OK"]
    assert _call(L, entry, M=0, p=0.0) == codes["OK"]


def test_act_bwd_identity_does_not_need_h(L, codes):
    lib = L.lib()
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = 0.1, 1, None
    good = L.PtrArr9()
    good[0] = 0x1000
    assert lib.mtlora_act_dropout_bwd(1, good, None, good, ctypes.byref(dr), 0x45, 0, 0, 16, L.F32, None) == codes["OK"]
    assert lib.mtlora_act_dropout_bwd(1, good, None, good, ctypes.byref(dr), 0x42, 1, 0, 16, L.F32, None) == codes["ERR_NULL"]


def _scratch_of(src, tmp_path):
    from mtlora_amd.csrc import build as B
    p = subprocess.run([B._hipcc()] + B.FLAGS + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                 os.path.join(B.HERE, src), "-o", str(tmp_path / (src + ".dev.o"))],
                       capture_output=True, text=True, cwd=B.HERE)
    assert p.returncode == 0, p.stderr[-2000:]
    scratch, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur is not None:
            scratch[cur] = int(m.group(1))
    return scratch


def test_new_kernels_use_no_scratch(L, tmp_path):
    """k_act_dropout (3 dtypes x identity / GELU x forward / backward = 12) and the DROP instantiations of k_residual_fwd / _bwd (7 dtype
    pairs each = 14) report 0 bytes of scratch per lane in the compiler's resource remarks, read as
    test_cpu_attention_dropout.py::test_new_kernels_use_no_scratch reads them; so do the 14 plain instantiations next to them."""
    act = {k: v for k, v in _scratch_of("act_dropout.hip", tmp_path).items() if "k_act_dropout" in k}
    print(sorted(act.items()))
    assert len(act) == 12 and all(v == 0 for v in act.values()), act
    res = {k: v for k, v in _scratch_of("glue.hip", tmp_path).items() if "k_residual_" in k}
    print(sorted(res.items()))
    drop = {k: v for k, v in res.items() if "Lb1E" in k}
    assert len(res) == 28 and len(drop) == 14, sorted(res)
    assert all(v == 0 for v in res.values()), {k: v for k, v in res.items() if v}
