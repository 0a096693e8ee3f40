"""Host side of the implicit task hiddens for task ranks 16 .. 128 (mtlora_mlp_hidr_*, csrc/hid_wide.h): exports, shape rules, size
queries and argument checks -- no GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mtlora_mlp_hidr_supported", "mtlora_mlp_hidr_fwd_scratch_bytes", "mtlora_mlp_hidr_bwd_scratch_bytes", "mtlora_mlp_hidr_proj",
         "mtlora_mlp_hidr_bwd"]


@pytest.fixture(scope="module")
def lib():
    from mtlora_amd.csrc.build import build
    from mtlora_amd import _lib
    return build(verbose=False), _lib.lib()


def _descs(r1=(16, 16), r2=(16, 16), M=200, C=64, H=256, dtype=None, M2=None, x_tasks=1):
    from mtlora_amd import _lib
    d1, d2 = _lib.LinearDesc(), _lib.LinearDesc()
    for d, K, N, r, m in ((d1, C, H, r1, M), (d2, H, C, r2, M if M2 is None else M2)):
        d.M, d.K, d.N, d.dtype, d.T, d.r_s, d.has_x_tasks = m, K, N, _lib.BF16 if dtype is None else dtype, len(r), 16, x_tasks
        for i, v in enumerate(r):
            d.r_t[i] = v
    return d1, d2


def test_exports_and_abi(lib):
    from mtlora_amd import _lib
    path, L = lib
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    nm = subprocess.run(["nm", "-D", path], capture_output=True, text=True).stdout
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", hdr) and n in _lib.EXPORTS and f" T {n}" in nm, n
    assert L.mtlora_version() == _lib.ABI_VERSION == 12


ACCEPT = {"r16": dict(r1=(16,), r2=(16,)), "r48": dict(r1=(48, 48), r2=(48, 48)), "r128": dict(r1=(128,) * 8, r2=(128,) * 8, C=128),
          "mixed": dict(r1=(16, 32), r2=(32, 16)), "H4096": dict(H=4096)}
REJECT = {"r8": dict(r1=(8, 8), r2=(8, 8)), "r24": dict(r1=(24, 16)), "r144": dict(r2=(16, 144), C=256), "H%128": dict(H=320),
          "T0": dict(r1=(), r2=()), "no_x_tasks": dict(x_tasks=0), "M mismatch": dict(M2=201)}


@pytest.mark.parametrize("case", list(ACCEPT) + list(REJECT) + ["fp32"])
def test_shape_rules(lib, case):
    """supported shapes answer 1 and positive sizes; every other one 0, -1 from both size queries and MTLORA_ERR_UNSUPPORTED (-7) from
    both launch entries (before any pointer is looked at); the r_t <= 8 entries keep rejecting rank 16."""
    from mtlora_amd import _lib
    L = lib[1]
    d1, d2 = _descs(**({"dtype": _lib.F32} if case == "fp32" else {**ACCEPT, **REJECT}[case]))
    a, b = ctypes.byref(d1), ctypes.byref(d2)
    ok = case in ACCEPT
    assert L.mtlora_mlp_hidr_supported(a, b) == int(ok)
    f, w = L.mtlora_mlp_hidr_fwd_scratch_bytes(a, b), L.mtlora_mlp_hidr_bwd_scratch_bytes(a, b)
    assert (f > 0 and w > 0) if ok else (f == -1 and w == -1)
    proj = L.mtlora_mlp_hidr_proj(a, b, None, None, None, None, 0, None)
    bwd = L.mtlora_mlp_hidr_bwd(a, b, None, None, None, None, None, None, None, None, None, None, 0, None)
    assert (proj, bwd) == ((-4, -4) if ok else (-7, -7))  # (supported shape, null pointers: MTLORA_ERR_NULL before any launch)
    if case != "r8":
        assert L.mtlora_mlp_hid_supported(a, b) == 0 and L.mtlora_mlp_hid_fwd_scratch_bytes(a, b) == -1
