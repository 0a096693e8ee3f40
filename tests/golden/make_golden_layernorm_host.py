"""Fixture that pins what the LayerNorm family's host dispatch (csrc/layernorm.hip) answers without a GPU.

    python tests/golden/make_golden_layernorm_host.py [--lib PATH] [--out tests/golden/layernorm_host.json]

scratch: mtlora_layernorm_bwd_scratch_bytes and mtlora_layernorm_multi_bwd_scratch_bytes over scratch_table(): every LPR (8, 16, 32,
         64), both sides of vpl <= 3, the grid cap (M large enough that the partial count saturates at 1024), M = 0, invalid C,
         invalid dtype, n in {0, 1, 2, 9, 10}.
reject : the return code of every exported LayerNorm entry for calls that are rejected on the host, ONE defect per row
         (reject_table()), plus the forward entries with M == 0 (OK without a launch).  Pointers are fake non-null integers that are
         never dereferenced; no row may reach a launch (the generator refuses a row that returns OK with M > 0, and the backward
         entries with M == 0 zero dgamma / dbeta on the device, so they are not in the table).  None of the public residual entries
         takes merge arguments it would reject, so there is no such row.
--lib points at another build of libmtlora_hip.so (the fixture is generated from the commit BEFORE a host-side refactor and must
hold after it); the test imports this module for the tables, so generator and test cannot drift apart.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mtlora_amd import _lib as L  # noqa: E402

F32, BF16, F16 = L.F32, L.BF16, L.F16
NMAX = L.MAX_TASKS + 1


# ------------------------------------------------------------------------------------------------
# scratch sizes
# ------------------------------------------------------------------------------------------------
SCRATCH_M = (0, 1, 7, 333, 4096, 100352, 10 ** 7, -1)
SCRATCH_C = (-8, 0, 8, 64, 66, 96, 100, 192, 200, 384, 768, 1024, 1536, 2048, 2052, 4096, 4104)
SCRATCH_DT = (F32, BF16, F16, 7)
SCRATCH_N = (0, 1, 2, 9, 10)


def scratch_table():
    for dt in SCRATCH_DT:
        for C in SCRATCH_C:
            for M in SCRATCH_M:
                yield f"dt{dt} C{C} M{M}", (M, C, dt)


def scratch_of(lib, M, C, dt):
    """[single query, multi query for every n of SCRATCH_N]"""
    return [lib.mtlora_layernorm_bwd_scratch_bytes(M, C, dt)] + [lib.mtlora_layernorm_multi_bwd_scratch_bytes(n, M, C, dt)
                                                                 for n in SCRATCH_N]


# ------------------------------------------------------------------------------------------------
# rejected calls.  An entry is its C parameter list: (name, kind[, flags]); kinds: "p" pointer, "a" per-stream pointer array,
# "i" integer, "f" float, "s" stream.  flags: R = null is rejected (an array: the array and each of its first n elements),
# r = a null ARRAY is rejected (its elements may be null), A = 16-byte alignment is checked.
# ------------------------------------------------------------------------------------------------
ENTRIES = {
    "mtlora_layernorm_fwd": [("x", "p", "RA"), ("gamma", "p", "R"), ("beta", "p", "R"), ("y", "p", "RA"), ("mean", "p", "R"),
                             ("rstd", "p", "R"), ("M", "i"), ("C", "i"), ("eps", "f"), ("x_dtype", "i"), ("o_dtype", "i"),
                             ("merge_h", "i"), ("merge_w", "i"), ("stream", "s")],
    "mtlora_residual_layernorm_fwd": [("x", "p", "RA"), ("branch", "p", "RA"), ("scale", "p", ""), ("B", "i"), ("gamma", "p", "R"),
                                      ("beta", "p", "R"), ("x_new", "p", "RA"), ("y", "p", "RA"), ("mean", "p", "R"),
                                      ("rstd", "p", "R"), ("M", "i"), ("C", "i"), ("eps", "f"), ("x_dtype", "i"), ("o_dtype", "i"),
                                      ("stream", "s")],
    "mtlora_layernorm_bwd": [("dy", "p", "RA"), ("x", "p", "RA"), ("gamma", "p", "R"), ("mean", "p", "R"), ("rstd", "p", "R"),
                             ("dx", "p", "RA"), ("dgamma", "p", "R"), ("dbeta", "p", "R"), ("M", "i"), ("C", "i"), ("x_dtype", "i"),
                             ("o_dtype", "i"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("dx_addend", "p", "A"),
                             ("merge_h", "i"), ("merge_w", "i"), ("stream", "s")],
    "mtlora_residual_layernorm_bwd": [("dy", "p", "RA"), ("x", "p", "RA"), ("gamma", "p", "R"), ("mean", "p", "R"),
                                      ("rstd", "p", "R"), ("dx", "p", "RA"), ("d_branch", "p", "RA"), ("dgamma", "p", "R"),
                                      ("dbeta", "p", "R"), ("scale", "p", ""), ("B", "i"), ("M", "i"), ("C", "i"), ("x_dtype", "i"),
                                      ("o_dtype", "i"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("dx_addend", "p", "A"),
                                      ("stream", "s")],
    "mtlora_layernorm_multi_fwd": [("n", "i"), ("x", "a", "RA"), ("gamma", "p", "R"), ("beta", "p", "R"), ("y", "a", "RA"),
                                   ("mean", "a", "R"), ("rstd", "a", "R"), ("M", "i"), ("C", "i"), ("eps", "f"), ("x_dtype", "i"),
                                   ("o_dtype", "i"), ("merge_h", "i"), ("merge_w", "i"), ("stream", "s")],
    "mtlora_layernorm_multi_bwd": [("n", "i"), ("dy", "a", "RA"), ("x", "a", "RA"), ("gamma", "p", "R"), ("mean", "a", "R"),
                                   ("rstd", "a", "R"), ("dx", "a", "RA"), ("dgamma", "p", "R"), ("dbeta", "p", "R"), ("M", "i"),
                                   ("C", "i"), ("x_dtype", "i"), ("o_dtype", "i"), ("scratch", "p", "RA"), ("scratch_bytes", "i"),
                                   ("dx_addend", "a", "A"), ("merge_h", "i"), ("merge_w", "i"), ("stream", "s")],
    "mtlora_residual_layernorm_streams_fwd": [("n", "i"), ("x", "a", "RA"), ("branch", "a", "RA"), ("scale", "p", ""), ("B", "i"),
                                              ("gamma", "p", "R"), ("beta", "p", "R"), ("x_new", "a", "RA"), ("y", "a", "RA"),
                                              ("mean", "a", "R"), ("rstd", "a", "R"), ("M", "i"), ("C", "i"), ("eps", "f"),
                                              ("x_dtype", "i"), ("o_dtype", "i"), ("merge_h", "i"), ("merge_w", "i"),
                                              ("stream", "s")],
    "mtlora_residual_layernorm_streams_bwd": [("n", "i"), ("dy", "a", "RA"), ("x", "a", "RA"), ("gamma", "p", "R"),
                                              ("mean", "a", "R"), ("rstd", "a", "R"), ("dx", "a", "RA"), ("d_branch", "a", "rA"),
                                              ("dgamma", "p", "R"), ("dbeta", "p", "R"), ("scale", "p", ""), ("B", "i"), ("M", "i"),
                                              ("C", "i"), ("x_dtype", "i"), ("o_dtype", "i"), ("scratch", "p", "RA"),
                                              ("scratch_bytes", "i"), ("dx_addend", "a", "A"), ("merge_h", "i"), ("merge_w", "i"),
                                              ("stream", "s")],
    "mtlora_residual_layernorm_multi_fwd": [("n", "i"), ("x", "p", "RA"), ("branch", "a", "RA"), ("scale", "p", ""), ("B", "i"),
                                            ("gamma", "p", "R"), ("beta", "p", "R"), ("x_new", "a", "RA"), ("y", "a", "RA"),
                                            ("mean", "a", "R"), ("rstd", "a", "R"), ("M", "i"), ("C", "i"), ("eps", "f"),
                                            ("x_dtype", "i"), ("o_dtype", "i"), ("stream", "s")],
    "mtlora_residual_layernorm_multi_bwd": [("n", "i"), ("dy", "a", "RA"), ("x", "a", "RA"), ("gamma", "p", "R"), ("mean", "a", "R"),
                                            ("rstd", "a", "R"), ("dx_addend", "a", "A"), ("dx", "p", "RA"), ("d_branch", "a", "A"),
                                            ("dgamma", "p", "R"), ("dbeta", "p", "R"), ("scale", "p", ""), ("B", "i"), ("M", "i"),
                                            ("C", "i"), ("x_dtype", "i"), ("o_dtype", "i"), ("scratch", "p", "RA"),
                                            ("scratch_bytes", "i"), ("stream", "s")],
}
GOOD = dict(n=3, M=12, C=64, B=3, eps=1e-5, x_dtype=F32, o_dtype=F32, merge_h=0, merge_w=0, scratch_bytes=1 << 40)


def _flags(param):
    return param[2] if len(param) > 2 else ""


def reject_table():
    """(key, entry, edits): the call is the entry's good call (GOOD; pointer j is the fake address 4096 * (j + 1), element k of array
    j is 4096 * (j + 1) + 64 * k) with `edits` applied: {name: value} for scalars, {name: None} a null pointer / array,
    {name: ("null", k)} / {name: ("odd", k)} element k of an array null / misaligned, {name: "odd"} a misaligned pointer,
    {"scratch_bytes": "short"} one byte less than the entry needs."""
    for entry, params in ENTRIES.items():
        names = [p[0] for p in params]
        fwd = entry.endswith("_fwd")
        rows = [("x_dtype 7", {"x_dtype": 7}), ("x_dtype -1", {"x_dtype": -1}), ("o_dtype 3", {"o_dtype": 3}),
                ("o_dtype -1", {"o_dtype": -1}), ("bf16 x f16", {"x_dtype": BF16, "o_dtype": F16}),
                ("f16 x bf16", {"x_dtype": F16, "o_dtype": BF16}), ("C 66", {"C": 66}), ("C 68 bf16", {"C": 68, "x_dtype": BF16}),
                ("C 0", {"C": 0}), ("C -64", {"C": -64}), ("M -1", {"M": -1}), ("C 2052 over", {"C": 2052}),
                ("C 4104 over f16", {"C": 4104, "x_dtype": F16}), ("C 4104 over bf16", {"C": 4104, "x_dtype": BF16, "o_dtype": BF16})]
        for p in params:
            name, kind, fl = p[0], p[1], _flags(p)
            if kind == "p":
                if "R" in fl:
                    rows.append((f"null {name}", {name: None}))
                if "A" in fl:
                    rows.append((f"odd {name}", {name: "odd"}))
            elif kind == "a":
                if "R" in fl or "r" in fl:
                    rows.append((f"null {name}[]", {name: None}))
                for k in (0, GOOD["n"] - 1):
                    if "R" in fl:
                        rows.append((f"null {name}[{k}]", {name: ("null", k)}))
                    if "A" in fl:
                        rows.append((f"odd {name}[{k}]", {name: ("odd", k)}))
        if "B" in names:
            rows += [("B 5", {"B": 5}), ("B 0", {"B": 0}), ("B -3", {"B": -3})]
        if "n" in names:
            rows += [("n 0", {"n": 0}), ("n -1", {"n": -1}), (f"n {NMAX + 1}", {"n": NMAX + 1})]
        if "merge_h" in names:
            rows += [("merge 3x2", {"merge_h": 3, "merge_w": 2}), ("merge 2x3", {"merge_h": 2, "merge_w": 3}),
                     ("merge 2x0", {"merge_h": 2, "merge_w": 0}), ("merge -2x2", {"merge_h": -2, "merge_w": 2}),
                     ("merge 4x10 rows", {"merge_h": 4, "merge_w": 10}), ("merge 2x2 C 8", {"merge_h": 2, "merge_w": 2, "C": 8}),
                     ("merge 2x2 C 80 bf16", {"merge_h": 2, "merge_w": 2, "C": 80, "x_dtype": BF16})]
        if "scratch_bytes" in names:
            rows += [("scratch short", {"scratch_bytes": "short"}), ("scratch 0", {"scratch_bytes": 0}),
                     ("scratch short C 1024 M 4099", {"scratch_bytes": "short", "C": 1024, "M": 4099 * 3}),
                     ("scratch -1", {"scratch_bytes": -1})]
        if fwd:  # no rows: OK without a launch
            rows += [("M 0", {"M": 0}), ("M 0 bf16", {"M": 0, "x_dtype": BF16, "o_dtype": BF16, "C": 4096})]
            if "merge_h" in names:
                rows.append(("M 0 merge 3x2", {"M": 0, "merge_h": 3, "merge_w": 2}))
        for what, edits in rows:
            yield f"{entry}: {what}", entry, edits


def call(lib, entry, edits):
    """the return code of `entry` for its good call with `edits` applied"""
    params = ENTRIES[entry]
    v = {**GOOD, **{k: e for k, e in edits.items() if not isinstance(e, (str, tuple)) and e is not None}}
    n_fill = GOOD["n"]
    args, keep = [], []
    for j, p in enumerate(params):
        name, kind = p[0], p[1]
        e = edits.get(name, "good") if kind in ("p", "a") else None
        base = 4096 * (j + 1)
        if kind == "p":
            args.append(None if e is None else ctypes.c_void_p(base + (4 if e == "odd" else 0)))
        elif kind == "a":
            if e is None:
                args.append(None)
                continue
            a = L.PtrArr9()
            for k in range(n_fill):
                a[k] = base + 64 * k
            if isinstance(e, tuple):
                a[e[1]] = None if e[0] == "null" else base + 64 * e[1] + 4
            keep.append(a)
            args.append(a)
        elif kind == "s":
            args.append(None)
        elif name == "scratch_bytes" and edits.get(name) == "short":
            q = (lib.mtlora_layernorm_multi_bwd_scratch_bytes(v["n"], v["M"], v["C"], v["x_dtype"])
                 if entry in ("mtlora_layernorm_multi_bwd", "mtlora_residual_layernorm_streams_bwd")
                 else lib.mtlora_layernorm_bwd_scratch_bytes(v["M"], v["C"], v["x_dtype"]))
            assert q > 256, (entry, edits, q)
            args.append(q - 256 - 1)  # (the queries return 256 bytes of slack the entries do not insist on)
        else:
            args.append(v[name])
    return getattr(lib, entry)(*args)


def gen(lib):
    scratch = {key: scratch_of(lib, *a) for key, a in scratch_table()}
    reject = {}
    for key, entry, edits in reject_table():
        assert key not in reject, key
        code = call(lib, entry, edits)
        assert code < 0 or edits.get("M") == 0, (key, code)  # a row that passed validation with rows to process reached a launch
        reject[key] = code
    return {"scratch_columns": ["bwd_scratch_bytes"] + [f"multi_bwd_scratch_bytes n={n}" for n in SCRATCH_N], "scratch": scratch,
            "reject": reject}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libmtlora_hip.so to load instead of the tree's own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "layernorm_host.json")
    with open(out, "w") as f:
        json.dump(gen(L.lib()), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
