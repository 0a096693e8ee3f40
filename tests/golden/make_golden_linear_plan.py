"""Fixture that pins what MTLoRALinear's host dispatch (csrc/linear.hip) ASKS for.

    python tests/golden/make_golden_linear_plan.py sizes [--lib PATH] [--out tests/golden/linear_sizes.json]

sizes (no GPU): for every descriptor of size_table() the workspace queries of include/mtlora_hip.h (ctx bytes, backward scratch
bytes, and -- the layer taken as fc1 of an Mlp whose fc2 is its mirror image -- mtlora_mlp_hid_supported and the two hid scratch
sizes).
--lib points at another build of libmtlora_hip.so (the fixture is generated from the commit BEFORE a host-side refactor and must
hold after it); the test imports this module for the table, so generator and test cannot drift apart.
"""
from __future__ import annotations

import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mtlora_amd import _lib as L  # noqa: E402

DT = {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}
MIXED = (4, 16, 32, 8)


def make_desc(M, K, N, dtype, T, r_s, r_t, mode, has_x_tasks) -> L.LinearDesc:
    d = L.LinearDesc()
    d.M, d.K, d.N = M, K, N
    d.dtype = DT[dtype]
    d.mode, d.T, d.r_s = mode, T, r_s
    for i in range(T):
        d.r_t[i] = r_t[i]
        d.scale_t[i] = 1.0
    d.scale_s = 1.0
    d.has_x_tasks = 1 if (has_x_tasks and T > 0) else 0
    return d


# ------------------------------------------------------------------------------------------------
# sizes
# ------------------------------------------------------------------------------------------------
def size_table():
    """(key, kwargs) in a fixed order.  T = 0 has no task ranks and no task inputs: one entry instead of eight."""
    for dtype, T, r_s, mode, (K, N), M in itertools.product(("f32", "bf16", "f16"), (0, 1, 4), (0, 8, 64), (0, 1),
                                                            ((96, 384), (384, 96), (192, 192), (1536, 384), (40, 1080)),
                                                            (0, 7, 333, 100352)):
        for rt, xt in (itertools.product((4, 16, 32, "mixed"), (False, True)) if T else (("-", False),)):
            r_t = () if not T else (MIXED[:T] if rt == "mixed" else (rt,) * T)
            key = f"{dtype} T{T} rs{r_s} rt{rt} mode{mode} xt{int(xt)} K{K} N{N} M{M}"
            yield key, dict(M=M, K=K, N=N, dtype=dtype, T=T, r_s=r_s, r_t=r_t, mode=mode, has_x_tasks=xt)


def sizes_of(lib, kw):
    d1 = make_desc(**kw)
    d2 = make_desc(**{**kw, "K": kw["N"], "N": kw["K"]})
    return [lib.mtlora_linear_ctx_bytes(ctypes.byref(d1)), lib.mtlora_linear_bwd_scratch_bytes(ctypes.byref(d1)),
            lib.mtlora_mlp_hid_supported(ctypes.byref(d1), ctypes.byref(d2)),
            lib.mtlora_mlp_hid_fwd_scratch_bytes(ctypes.byref(d1), ctypes.byref(d2)),
            lib.mtlora_mlp_hid_bwd_scratch_bytes(ctypes.byref(d1), ctypes.byref(d2))]


def gen_sizes(lib):
    """entry i of size_table() has the sizes values[index[i]] (the 6120 entries share a few hundred distinct rows)"""
    values, index = [], []
    for _key, kw in size_table():
        row = sizes_of(lib, kw)
        if row not in values:
            values.append(row)
        index.append(values.index(row))
    return {"columns": ["ctx_bytes", "bwd_scratch_bytes", "hid_supported", "hid_fwd_scratch_bytes", "hid_bwd_scratch_bytes"],
            "values": values, "index": index}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sizes"])
    ap.add_argument("--lib", default=None, help="libmtlora_hip.so to load instead of the tree's own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "linear_sizes.json")
    with open(out, "w") as f:
        json.dump(gen_sizes(L.lib()), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
