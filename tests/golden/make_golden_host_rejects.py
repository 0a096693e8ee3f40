"""Fixture that pins the return code of every entry point whose host dispatch goes through csrc/dispatch.h, without a GPU.

    python tests/golden/make_golden_host_rejects.py [--lib PATH] [--out tests/golden/host_rejects.json]

Every row of reject_table() is the entry's smallest valid call (its GOOD values; pointers are fake non-null integers that are never
dereferenced: pointer j is 4096 * (j + 1), element k of array j is 4096 * (j + 1) + 64 * k) with ONE defect: a dtype code outside the
entry's set, a null pointer / array / array element, a pointer or array element off by 4 or by 8 bytes, a bad extent, n out of range,
B not dividing the rows, a workspace one byte short; plus one call without rows per entry.  No row may reach a launch: gen() refuses
a row that returns MTLORA_OK unless it is marked as a call without work, and any row that returns MTLORA_ERR_HIP (a launch that
failed for want of a device).

dtype sweeps set the argument to -1, every defined code (fp32, bf16, fp16, uint8) and one past the last.  An accepted code would
launch, so the sweep is made on a call that stops right after the dtype test: the call without rows where the entry returns OK for
it, else a defect that is tested later (the entry's `stop` edit: a null pointer, or a short workspace) -- the row then records
"accepted" as that later code and "rejected" as MTLORA_ERR_DTYPE, which pins the accepted set all the same.

--lib points at another build of libmtlora_hip.so: the fixture is recorded from the commit BEFORE the host-dispatch refactor and
must hold after it.  The test imports this module for the table, so generator and test cannot drift apart.

Rows that are NOT in the table because the library accepts the defective call and would launch (the lax spots; tightening one is a
behaviour change of its own):
  * alignment is not tested at all by mtlora_upsample_loss, mtlora_upsample_metrics (the kernels read scalars / 8-byte rows), nor for
    gamma / beta / the save_* / dgamma / dbeta / mean / rstd fp32 vectors of the BatchNorm entries, `out` of mtlora_colsum,
    `out` and `scratch` of mtlora_label_stat, `bias` / `dbias` / `mask` / `mask_ids` of window attention, the fp32 masters of the
    pack entries, the factor gradients of mtlora_linear_bwd, dB1_t / dA2_t of mtlora_mlp_hid_bwd;
  * mtlora_upsample_predict tests `out` for 4 bytes only (fp32 output), and `out` of mtlora_gemm_tn likewise: off by 4 or 8 passes;
  * mtlora_upsample_cl_fwd / _bwd accept pointers off by 8 for the 16-bit types, mtlora_linear_pack_table a table off by 8;
  * mtlora_residual_droppath_bwd accepts null elements of g and dy and does not test dres; `scale` may be null everywhere;
  * running_mean / running_var (BatchNorm), mask / mask_ids (attention), bias, dy_s, dy_t, dx_t, dA_* / dB_* (linear backward),
    dh_s, dB1_t, dA2_t (hid backward) are optional: null is a valid call;
  * a call without rows still launches in mtlora_colsum (M = 0 sums to zeros), mtlora_gemm_tn, mtlora_window_attn_bwd / _drop_bwd
    (they zero their outputs): these have no "no rows" row, their dtype sweep stops at a later defect;
  * mtlora_linear_bwd_gelu with a null descriptor reads d->T before any test (it would crash, not launch): no such row.
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

F32, BF16, F16, U8 = L.F32, L.BF16, L.F16, 3
DT_CODES = (-1, F32, BF16, F16, U8, U8 + 1)
NMAX = L.MAX_TASKS + 1
BIG = 1 << 40
ERR_HIP = -6

# descriptor defaults ("L": mtlora_linear_desc, "T": mtlora_attn_desc, "O": mtlora_attn_dropout); a parameter of such a kind takes
# its fields from the values "<param>.<field>"
DESC = {
    "L": (L.LinearDesc, dict(M=8, K=8, N=8, dtype=F32, mode=0, T=2, r_s=4, r_t=(4, 4), scale_s=1.0, scale_t=(1.0, 1.0), has_x_tasks=1,
                             dropout_p=0.0, seed=1, seed_offset=None, bwd_phase=0, sel_stream=0, sel_dense=0, sel_tn=0, sel_projk=0,
                             max_cu=0, packed=None, hid=0, hid_ptr=None)),
    "T": (L.AttnDesc, dict(B=1, H=2, W=2, window_size=2, shift=0, num_heads=1, head_dim=32, image_layout=0, dtype=F32, scale=1.0,
                           mask_value=-100.0)),
    "O": (L.AttnDropout, dict(p=0.1, seed=1, seed_offset=None)),
}

# ------------------------------------------------------------------------------------------------
# An entry: params = its C parameter list as (name, kind, flags).  kinds: "p" pointer, "a" pointer array, "i" integer, "f" float,
# "s" stream, "h" a writable host buffer, "L" / "T" / "O" descriptor.  flags: R = null is rejected (an array: the array and its elements), r = a null ARRAY is
# rejected (elements may be null), A = 16-byte alignment is tested (off by 4 and by 8 are rejected), 8 = 8-byte alignment (off by 4).
# good: the scalars of the valid call;  n: the value that counts array elements;  dtypes: the dtype arguments (a tuple is set
# together);  stop / stop_ok: the edit the dtype sweep adds, and whether it makes a call without work (OK allowed);
# short: {byte-count argument: needed bytes};  rows: further (what, edits[, no_work]) rows.
# ------------------------------------------------------------------------------------------------
def _q(fn, *names, slack=256):
    """needed bytes = size query over the named values / descriptors, minus the slack the query adds"""
    return lambda lib, v, d: getattr(lib, fn)(*[d[n] if n in d else v[n] for n in names]) - slack


_LIN_DESC_ROWS = [("K 6", {"K": 6}), ("N 6", {"N": 6}), ("K 12 bf16", {"K": 12, "dtype": BF16}), ("K 0", {"K": 0}), ("N -8", {"N": -8}),
                  ("M -1", {"M": -1}), ("M 2^31", {"M": 1 << 31}), ("T 9", {"T": L.MAX_TASKS + 1}), ("T -1", {"T": -1}),
                  ("r_s -1", {"r_s": -1}), ("r_t 0", {"r_t": (4, 0)}), ("mode 2", {"mode": 2}), ("bwd_phase 3", {"bwd_phase": 3}),
                  ("sel_stream 2", {"sel_stream": 2}), ("sel_dense 5", {"sel_dense": 5}), ("max_cu -1", {"max_cu": -1}),
                  ("dropout_p 1", {"dropout_p": 1.0})]


def _lin_rows(prefix, r_t=(4, 0)):
    """the descriptor defects of check_desc; r_t: a rank tuple with a zero among the first T"""
    return [(f"{prefix}.{w}", {f"{prefix}.{k}": (r_t if k == "r_t" else e) for k, e in ed.items()}) for w, ed in _LIN_DESC_ROWS]


_ATTN_ROWS = [("head_dim 64", {"d.head_dim": 64}), ("window 0", {"d.window_size": 0}), ("window 13", {"d.window_size": 13, "d.H": 13, "d.W": 13}),
              ("B -1", {"d.B": -1}), ("H 0", {"d.H": 0}), ("H 3", {"d.H": 3}), ("W 3", {"d.W": 3}), ("heads 0", {"d.num_heads": 0}),
              ("shift 2", {"d.shift": 2}), ("shift -1", {"d.shift": -1}), ("rows 2^31", {"d.B": 1 << 29})]
_DROP_ROWS = [("p 1", {"drop.p": 1.0}), ("p -0.5", {"drop.p": -0.5}), ("p nan", {"drop.p": float("nan")}), ("p inf", {"drop.p": float("inf")})]
_UP = dict(B=1, h=2, w=2, C=4, scale=2, dtype=F32)
_UP_ROWS = [("B -1", {"B": -1}), ("h 0", {"h": 0}), ("w -2", {"w": -2}), ("C 0", {"C": 0}), ("scale 0", {"scale": 0})]
_BN = dict(R=64, C=8, dtype=F32, momentum=0.1, eps=1e-5, relu=1, scratch_bytes=BIG)
_BN_ROWS = [("R 0", {"R": 0}, True), ("R -1", {"R": -1}), ("C 0", {"C": 0}), ("C -8", {"C": -8}), ("C 6", {"C": 6}),
            ("C 12 bf16", {"C": 12, "dtype": BF16}), ("C 12 f16", {"C": 12, "dtype": F16}), ("C 2052 over", {"C": 2052}),
            ("C 4104 over bf16", {"C": 4104, "dtype": BF16})]
_RES = dict(n=2, M=64, C=8, B=2, res_dtype=F32, y_dtype=F32)
_RES_ROWS = ([(f"pair {a}x{b}", {"res_dtype": a, "y_dtype": b, "M": 0}, True) for a in (F32, BF16, F16) for b in (F32, BF16, F16)] +
             [("n 0", {"n": 0}), ("n -1", {"n": -1}), (f"n {NMAX + 1}", {"n": NMAX + 1}), ("M -1", {"M": -1}), ("C 0", {"C": 0}),
              ("C -8", {"C": -8}), ("C 4", {"C": 4}), ("C 12", {"C": 12}), ("B 0", {"B": 0}), ("B -2", {"B": -2}), ("B 3", {"B": 3}),
              ("M 0", {"M": 0}, True)])
_LIN_FWD = [("d", "L", "R"), ("x", "p", "RA"), ("x_t", "a", "RA"), ("W", "p", "RA"), ("bias", "p", "A"), ("A_s", "p", "R"), ("B_s", "p", "R"),
            ("A_t", "a", "R"), ("B_t", "a", "R"), ("y_s", "p", "RA"), ("y_t", "a", "RA")]
_LIN_BWD = [("d", "L", "R"), ("x", "p", "RA"), ("x_t", "a", "RA"), ("Wt", "p", "RA"), ("dy_s", "p", "A"), ("dy_t", "a", "A"), ("ctx", "p", "RA"),
            ("ctx_bytes", "i"), ("dx", "p", "A"), ("dx_t", "a", "A"), ("dA_s", "p", ""), ("dB_s", "p", ""), ("dA_t", "a", ""), ("dB_t", "a", ""),
            ("scratch", "p", "RA"), ("scratch_bytes", "i")]
_LIN_GOOD = dict(ctx_bytes=BIG, scratch_bytes=BIG)
_LIN_FWD_ROWS = _lin_rows("d") + [("packed off 4", {"d.packed": 0x70004}), ("packed off 8", {"d.packed": 0x70008}),
                                  ("hid base null", {"d.hid": L.HID_FWD_BASE}), ("hid base off 4", {"d.hid": L.HID_FWD_BASE, "d.hid_ptr": 0x70004}),
                                  ("hid p matrixv2", {"d.hid": L.HID_P_GIVEN, "d.mode": 1}), ("M 0", {"d.M": 0}, True)]
_LIN_BWD_ROWS = _lin_rows("d") + [("hid q matrixv2", {"d.hid": L.HID_Q_GIVEN, "d.mode": 1}),
                                  ("hid q off 4", {"d.hid": L.HID_Q_GIVEN, "d.hid_ptr": 0x70004}), ("M 0", {"d.M": 0}, True)]
_CTX = _q("mtlora_linear_ctx_bytes", "d")
_HID1 = {"d1.K": 8, "d1.N": 128, "d1.dtype": BF16, "d1.T": 1, "d1.r_t": (4,), "d2.K": 128, "d2.N": 8, "d2.dtype": BF16, "d2.T": 1,
         "d2.r_t": (4,), "d2.packed": 0x90000}
_HID_ROWS = (_lin_rows("d1", (0,)) + [("d2.K 6", {"d2.K": 6}), ("d2 f16 x bf16", {"d2.dtype": F16}), ("M differs", {"d2.M": 16}),
                                ("N x K", {"d2.K": 256}), ("T differs", {"d2.T": 2, "d2.r_t": (4, 4)}), ("d1.T 0", {"d1.T": 0, "d2.T": 0}),
                                ("d1 matrixv2", {"d1.mode": 1}), ("d2 no x_tasks", {"d2.has_x_tasks": 0}), ("N 136", {"d1.N": 136, "d2.K": 136}),
                                ("r_t 9", {"d1.r_t": (9,)}), ("d2.r_t 16", {"d2.r_t": (16,)}),
                                ("N 2176 r 8", {"d1.N": 2176, "d2.K": 2176, "d1.r_t": (8,)}),
                                ("N 2176 tiled only", {"d1.N": 2176, "d2.K": 2176, "d1.sel_stream": 1}),
                                ("M 0", {"d1.M": 0, "d2.M": 0}, True), ("d1.packed off 4", {"d1.packed": 0x70004}),
                                ("d1.packed off 8", {"d1.packed": 0x70008})])

ENTRIES = {
    "mtlora_bn_relu_fwd": dict(
        params=[("x", "p", "RA"), ("gamma", "p", "R"), ("beta", "p", "R"), ("running_mean", "p", ""), ("running_var", "p", ""),
                ("momentum", "f"), ("eps", "f"), ("relu", "i"), ("y", "p", "RA"), ("save_mean", "p", "R"), ("save_rstd", "p", "R"),
                ("save_scale", "p", "R"), ("save_shift", "p", "R"), ("R", "i"), ("C", "i"), ("dtype", "i"), ("scratch", "p", "RA"),
                ("scratch_bytes", "i"), ("stream", "s")],
        good=_BN, dtypes=["dtype"], stop={"scratch_bytes": "short"}, rows=_BN_ROWS,
        short={"scratch_bytes": _q("mtlora_bn_scratch_bytes", "R", "C", "dtype")}),
    "mtlora_bn_relu_bwd": dict(
        params=[("dy", "p", "RA"), ("x", "p", "RA"), ("save_mean", "p", "R"), ("save_rstd", "p", "R"), ("save_scale", "p", "R"),
                ("save_shift", "p", "R"), ("relu", "i"), ("dx", "p", "RA"), ("dgamma", "p", "R"), ("dbeta", "p", "R"), ("R", "i"), ("C", "i"),
                ("dtype", "i"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("stream", "s")],
        good=_BN, dtypes=["dtype"], stop={"scratch_bytes": "short"}, rows=_BN_ROWS,
        short={"scratch_bytes": _q("mtlora_bn_scratch_bytes", "R", "C", "dtype")}),
    "mtlora_residual_droppath_fwd": dict(
        params=[("n", "i"), ("res", "a", "RA"), ("y", "a", "RA"), ("out", "a", "RA"), ("scale", "p", ""), ("M", "i"), ("C", "i"), ("B", "i"),
                ("res_dtype", "i"), ("y_dtype", "i"), ("stream", "s")],
        good=_RES, n="n", dtypes=["res_dtype", "y_dtype"], stop={"M": 0}, stop_ok=True, rows=_RES_ROWS),
    "mtlora_residual_droppath_bwd": dict(
        params=[("n", "i"), ("g", "a", "rA"), ("dy", "a", "rA"), ("dres", "p", ""), ("scale", "p", ""), ("M", "i"), ("C", "i"), ("B", "i"),
                ("res_dtype", "i"), ("y_dtype", "i"), ("stream", "s")],
        good=_RES, n="n", dtypes=["res_dtype", "y_dtype"], stop={"M": 0}, stop_ok=True, rows=_RES_ROWS),
    "mtlora_upsample_cl_fwd": dict(
        params=[("coarse", "p", "RA"), ("fine", "p", "RA"), ("B", "i"), ("h", "i"), ("w", "i"), ("C", "i"), ("scale", "i"), ("ld_fine", "i"),
                ("dtype", "i"), ("stream", "s")],
        good=dict(_UP, ld_fine=4), dtypes=["dtype"], stop={"B": 0}, stop_ok=True,
        rows=_UP_ROWS + [("ld 2", {"ld_fine": 2}), ("ld 6", {"ld_fine": 6, "C": 4}), ("C 6", {"C": 6, "ld_fine": 8}), ("B 2^38", {"B": 1 << 38}),
                         ("bf16 coarse off 4", {"dtype": BF16, "coarse": ("off", 4)}), ("f16 fine off 4", {"dtype": F16, "fine": ("off", 4)}),
                         ("B 0", {"B": 0}, True), ("B 0 null", {"B": 0, "coarse": None, "fine": None}, True)]),
    "mtlora_upsample_cl_bwd": dict(
        params=[("grad_fine", "p", "RA"), ("grad_coarse", "p", "RA"), ("B", "i"), ("h", "i"), ("w", "i"), ("C", "i"), ("scale", "i"), ("ld_fine", "i"),
                ("dtype", "i"), ("stream", "s")],
        good=dict(_UP, ld_fine=4), dtypes=["dtype"], stop={"B": 0}, stop_ok=True,
        rows=_UP_ROWS + [("ld 2", {"ld_fine": 2}), ("ld 6", {"ld_fine": 6, "C": 4}), ("C 6", {"C": 6, "ld_fine": 8}), ("B 2^38", {"B": 1 << 38}),
                         ("bf16 grad_fine off 4", {"dtype": BF16, "grad_fine": ("off", 4)}), ("f16 grad_coarse off 4", {"dtype": F16, "grad_coarse": ("off", 4)}),
                         ("B 0", {"B": 0}, True), ("B 0 null", {"B": 0, "grad_fine": None, "grad_coarse": None}, True)]),
    "mtlora_upsample_loss": dict(
        params=[("kind", "i"), ("low", "p", "R"), ("label", "p", "R"), ("stat", "p", "R"), ("dlow", "p", "R"), ("partials", "p", "R"),
                ("B", "i"), ("h", "i"), ("w", "i"), ("C", "i"), ("scale", "i"), ("dtype", "i"), ("ignore_index", "f"), ("stream", "s")],
        good=dict(_UP, kind=0, ignore_index=255.0), dtypes=["dtype"], stop={"B": 0}, stop_ok=True,
        rows=_UP_ROWS + [("scale 33", {"scale": 33}), ("kind 4", {"kind": 4}), ("kind -1", {"kind": -1}), ("kind 0 C 49", {"C": 49}),
                         ("kind 1 C 5", {"kind": 1, "C": 5}), ("kind 2 C 2", {"kind": 2, "C": 2}), ("kind 3 C 2", {"kind": 3, "C": 2}),
                         ("rows 2^31", {"h": 1 << 16, "w": 1 << 15, "scale": 1}), ("B 0", {"B": 0}, True)]),
    "mtlora_upsample_metrics": dict(
        params=[("kind", "i"), ("low", "p", "R"), ("label", "p", "R"), ("stat", "p", "R"), ("counts", "p", "R"), ("fpartials", "p", "R"),
                ("B", "i"), ("h", "i"), ("w", "i"), ("C", "i"), ("scale", "i"), ("dtype", "i"), ("ignore_index", "f"), ("stream", "s")],
        good=dict(_UP, kind=0, ignore_index=255.0), dtypes=["dtype"], stop={"B": 0}, stop_ok=True,
        rows=_UP_ROWS + [("scale 33", {"scale": 33}), ("kind 5", {"kind": 5}), ("kind -1", {"kind": -1}), ("kind 0 C 49", {"C": 49}),
                         ("kind 1 C 5", {"kind": 1, "C": 5}), ("kind 2 C 2", {"kind": 2, "C": 2}), ("kind 4 C 2", {"kind": 4, "C": 2}),
                         ("rows 2^31", {"h": 1 << 16, "w": 1 << 15, "scale": 1}), ("B 0", {"B": 0}, True)]),
    "mtlora_upsample_predict": dict(
        params=[("kind", "i"), ("low", "p", "R"), ("out", "p", "R"), ("B", "i"), ("h", "i"), ("w", "i"), ("C", "i"), ("scale", "i"),
                ("dtype", "i"), ("out_dtype", "i"), ("stream", "s")],
        good=dict(_UP, kind=1, out_dtype=F32), dtypes=["dtype", "out_dtype"], stop={"B": 0}, stop_ok=True,
        rows=[r for r in _UP_ROWS if r[0] != "scale 0"] + [
            ("scale 0", {"scale": 0}), ("scale 33", {"scale": 33}), ("kind 4", {"kind": 4}), ("kind -1", {"kind": -1}), ("kind 0 C 49", {"kind": 0, "C": 49, "out_dtype": U8}),
            ("kind 1 C 5", {"C": 5}), ("kind 2 C 2", {"kind": 2, "C": 2}), ("kind 0 f32 out", {"kind": 0}), ("kind 3 u8 out", {"kind": 3, "C": 1, "out_dtype": U8}),
            ("out off 2", {"out": ("off", 2)}), ("out off 1", {"out": ("off", 1)}), ("rows 2^31", {"h": 1 << 16, "w": 1 << 15, "scale": 1}),
            ("B 0", {"B": 0}, True)]),
    "mtlora_colsum": dict(
        params=[("x", "p", "RA"), ("M", "i"), ("N", "i"), ("dtype", "i"), ("out", "p", "R"), ("scratch", "p", "RA"), ("scratch_bytes", "i"),
                ("stream", "s")],
        good=dict(M=8, N=8, dtype=F32, scratch_bytes=BIG), dtypes=["dtype"], stop={"x": None},
        short={"scratch_bytes": _q("mtlora_colsum_scratch_bytes", "M", "N", slack=0)},
        rows=[("M -1", {"M": -1}), ("N 0", {"N": 0}), ("N -8", {"N": -8}), ("N 6", {"N": 6}), ("N 12 bf16", {"N": 12, "dtype": BF16}),
              ("N 2^20 + 8", {"N": (1 << 20) + 8}), ("scratch 0", {"scratch_bytes": 0})]),
    "mtlora_label_stat": dict(
        params=[("label", "p", "RA"), ("n", "i"), ("kind", "i"), ("ignore_index", "f"), ("out", "p", "R"), ("scratch", "p", "R"),
                ("scratch_bytes", "i"), ("stream", "s")],
        good=dict(n=8, kind=0, ignore_index=255.0, scratch_bytes=BIG), dtypes=[],
        short={"scratch_bytes": _q("mtlora_label_stat_scratch_bytes", "n", slack=0)},
        rows=[("n 0", {"n": 0}, True), ("n -1", {"n": -1}), ("kind 2", {"kind": 2}), ("kind -1", {"kind": -1}), ("scratch 0", {"scratch_bytes": 0})]),
    "mtlora_linear_pack": dict(
        params=[("d", "L", "R"), ("A_s", "p", "R"), ("B_s", "p", "R"), ("A_t", "a", "R"), ("B_t", "a", "R"), ("packed", "p", "RA"),
                ("packed_bytes", "i"), ("stream", "s")],
        good=dict(packed_bytes=BIG), n="d.T", dtypes=["d.dtype"], stop={"d.r_s": 0, "d.T": 0}, stop_ok=True,
        short={"packed_bytes": _q("mtlora_linear_packed_bytes", "d")},
        rows=_lin_rows("d") + [("nothing to pack", {"d.r_s": 0, "d.T": 0}, True), ("packed_bytes 0", {"packed_bytes": 0})]),
    "mtlora_linear_pack_entry": dict(  # (launches nothing; a valid call writes the entry, so entry_host is a real host buffer)
        params=[("d", "L", "R"), ("A_s", "p", "R"), ("B_s", "p", "R"), ("A_t", "a", "R"), ("B_t", "a", "R"), ("packed", "p", "RA"),
                ("packed_bytes", "i"), ("entry_host", "h", "R")],
        good=dict(packed_bytes=BIG), n="d.T", dtypes=["d.dtype"], stop={"entry_host": None},
        short={"packed_bytes": _q("mtlora_linear_packed_bytes", "d")},
        rows=_lin_rows("d") + [("nothing to pack", {"d.r_s": 0, "d.T": 0}), ("packed_bytes 0", {"packed_bytes": 0})]),
    "mtlora_linear_pack_table": dict(
        params=[("table_dev", "p", "R8"), ("n_entries", "i"), ("dtype", "i"), ("stream", "s")],
        good=dict(n_entries=1, dtype=F32), dtypes=["dtype"], stop={"n_entries": 0}, stop_ok=True,
        rows=[("n -1", {"n_entries": -1}), ("n 65536", {"n_entries": 65536}), ("n 0", {"n_entries": 0}, True),
              ("n 0 null", {"n_entries": 0, "table_dev": None}, True)]),
    "mtlora_gemm_tn": dict(
        params=[("a", "p", "RA"), ("b", "p", "RA"), ("out", "p", "R"), ("M", "i"), ("Na", "i"), ("Nb", "i"), ("lda", "i"), ("ldb", "i"),
                ("dtype", "i"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("stream", "s")],
        good=dict(M=8, Na=8, Nb=8, lda=8, ldb=8, dtype=F32, scratch_bytes=BIG), dtypes=["dtype"], stop={"scratch_bytes": "short"},
        short={"scratch_bytes": _q("mtlora_gemm_tn_scratch_bytes", "M", "Na", "Nb")},
        rows=[("M -1", {"M": -1}), ("M 2^31", {"M": 1 << 31}), ("Na 0", {"Na": 0}), ("Nb -8", {"Nb": -8}), ("lda 4", {"lda": 4}),
              ("ldb 4", {"ldb": 4}), ("Na 6", {"Na": 6}), ("Nb 6", {"Nb": 6}), ("lda 10", {"lda": 10}), ("ldb 10", {"ldb": 10}),
              ("Na 12 bf16", {"Na": 12, "lda": 16, "dtype": BF16}), ("Na 1032", {"Na": 1032, "lda": 1032}), ("out off 2", {"out": ("off", 2)}),
              ("scratch 0", {"scratch_bytes": 0})]),
    "mtlora_window_attn_fwd": dict(
        params=[("d", "T", "R"), ("qkv", "p", "RA"), ("bias", "p", "R"), ("mask", "p", ""), ("mask_ids", "p", ""), ("out", "p", "RA"),
                ("stream", "s")],
        good={}, dtypes=["d.dtype"], stop={"d.B": 0}, stop_ok=True, rows=_ATTN_ROWS + [("B 0", {"d.B": 0}, True)]),
    "mtlora_window_attn_drop_fwd": dict(
        params=[("d", "T", "R"), ("drop", "O", "R"), ("qkv", "p", "RA"), ("bias", "p", "R"), ("mask", "p", ""), ("mask_ids", "p", ""),
                ("out", "p", "RA"), ("stream", "s")],
        good={}, dtypes=["d.dtype"], stop={"d.B": 0}, stop_ok=True, rows=_ATTN_ROWS + _DROP_ROWS + [("B 0", {"d.B": 0}, True)]),
    "mtlora_window_attn_bwd": dict(
        params=[("d", "T", "R"), ("qkv", "p", "RA"), ("bias", "p", "R"), ("mask", "p", ""), ("mask_ids", "p", ""), ("dout", "p", "RA"),
                ("dqkv", "p", "RA"), ("dbias", "p", "R"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("stream", "s")],
        good=dict(scratch_bytes=BIG), dtypes=["d.dtype"], stop={"scratch_bytes": "short"},
        short={"scratch_bytes": _q("mtlora_window_attn_bwd_scratch_bytes", "d")}, rows=_ATTN_ROWS + [("scratch 0", {"scratch_bytes": 0})]),
    "mtlora_window_attn_drop_bwd": dict(
        params=[("d", "T", "R"), ("drop", "O", "R"), ("qkv", "p", "RA"), ("bias", "p", "R"), ("mask", "p", ""), ("mask_ids", "p", ""),
                ("dout", "p", "RA"), ("dqkv", "p", "RA"), ("dbias", "p", "R"), ("scratch", "p", "RA"), ("scratch_bytes", "i"), ("stream", "s")],
        good=dict(scratch_bytes=BIG), dtypes=["d.dtype"], stop={"scratch_bytes": "short"},
        short={"scratch_bytes": _q("mtlora_window_attn_bwd_scratch_bytes", "d")},
        rows=_ATTN_ROWS + _DROP_ROWS + [("scratch 0", {"scratch_bytes": 0})]),
    "mtlora_mlp_hid_proj": dict(
        params=[("d1", "L", "R"), ("d2", "L", "R"), ("h_base", "p", "RA"), ("ctx1", "p", "RA"), ("ctx2", "p", "RA"), ("scratch", "p", "RA"),
                ("scratch_bytes", "i"), ("stream", "s")],
        good=dict(_HID1, scratch_bytes=BIG), dtypes=[("d1.dtype", "d2.dtype"), "d1.dtype"], stop={"scratch": None},
        short={"scratch_bytes": _q("mtlora_mlp_hid_fwd_scratch_bytes", "d1", "d2", slack=0)},
        rows=_HID_ROWS + [("d2.packed null", {"d2.packed": None}), ("d2.packed off 4", {"d2.packed": 0x90004}),
                          ("d2.packed off 8", {"d2.packed": 0x90008})]),
    "mtlora_mlp_hid_bwd": dict(
        params=[("d1", "L", "R"), ("d2", "L", "R"), ("h_base", "p", "RA"), ("dh_s", "p", "A"), ("ctx1", "p", "RA"), ("ctx2", "p", "RA"),
                ("scratch2", "p", "RA"), ("scratch1", "p", "RA"), ("g", "p", "RA"), ("dB1_t", "a", ""), ("dA2_t", "a", ""), ("part", "p", "RA"),
                ("part_bytes", "i"), ("stream", "s")],
        good=dict(_HID1, part_bytes=BIG), n="d1.T", dtypes=[("d1.dtype", "d2.dtype"), "d1.dtype"], stop={"part": None},
        short={"part_bytes": _q("mtlora_mlp_hid_bwd_scratch_bytes", "d1", "d2", slack=0)},
        rows=[r for r in _HID_ROWS if not r[0].startswith("d1.packed")]),
    "mtlora_linear_fwd": dict(
        params=_LIN_FWD + [("ctx", "p", "RA"), ("ctx_bytes", "i"), ("stream", "s")],
        good=_LIN_GOOD, n="d.T", dtypes=["d.dtype"], stop={"d.M": 0}, stop_ok=True, short={"ctx_bytes": _CTX}, rows=_LIN_FWD_ROWS),
    "mtlora_linear_fwd_gelu": dict(
        params=_LIN_FWD + [("a_s", "p", "RA"), ("a_t", "a", "RA"), ("ctx", "p", "RA"), ("ctx_bytes", "i"), ("stream", "s")],
        good=_LIN_GOOD, n="d.T", dtypes=["d.dtype"], stop={"d.M": 0}, stop_ok=True, short={"ctx_bytes": _CTX}, rows=_LIN_FWD_ROWS),
    "mtlora_linear_bwd": dict(
        params=_LIN_BWD + [("stream", "s")],
        good=_LIN_GOOD, n="d.T", dtypes=["d.dtype"], stop={"d.M": 0}, stop_ok=True,
        short={"ctx_bytes": _CTX, "scratch_bytes": _q("mtlora_linear_bwd_scratch_bytes", "d")}, rows=_LIN_BWD_ROWS),
    "mtlora_linear_bwd_gelu": dict(
        params=[p if p[0] != "dx" else ("dx", "p", "RA") for p in _LIN_BWD] + [("h_s", "p", "RA"), ("h_t", "a", "RA"), ("stream", "s")],
        good=_LIN_GOOD, n="d.T", dtypes=["d.dtype"], stop={"d.M": 0}, stop_ok=True, no_null=("d",),
        short={"ctx_bytes": _CTX, "scratch_bytes": _q("mtlora_linear_bwd_scratch_bytes", "d")}, rows=_LIN_BWD_ROWS),
}


def _good(entry):
    """the scalars of the entry's valid call: descriptor defaults under "<param>.<field>", then the entry's own values"""
    v = {}
    for name, kind, *_ in ENTRIES[entry]["params"]:
        if kind in DESC:
            v.update({f"{name}.{f}": x for f, x in DESC[kind][1].items()})
    v.update(ENTRIES[entry]["good"])
    return v


def reject_table():
    """(key, entry, edits, no_work).  edits: {name: value} a scalar or descriptor field, {name: None} a null pointer / array /
    descriptor, {name: ("off", b)} a pointer off by b bytes, {name: ("null", k)} / {name: ("off", b, k)} element k of an array null /
    off by b bytes, {bytes argument: "short"} one byte less than the entry needs.  no_work: the call has nothing to launch, so
    MTLORA_OK is a legitimate answer."""
    for entry, E in ENTRIES.items():
        good = _good(entry)
        k = good[E["n"]] - 1 if "n" in E else 0  # the array element that gets the defect: the last one in use
        rows = []
        for names in E["dtypes"]:
            names = (names,) if isinstance(names, str) else names
            for code in DT_CODES:
                rows.append((f"{'+'.join(names)} {code}", {**{n: code for n in names}, **E["stop"]}, E.get("stop_ok", False)))
        for name, kind, *fl in E["params"]:
            fl = fl[0] if fl else ""
            if kind in DESC and "R" in fl and name not in E.get("no_null", ()):
                rows.append((f"null {name}", {name: None}))
            elif kind in ("p", "h"):
                if "R" in fl:
                    rows.append((f"null {name}", {name: None}))
                for b in ((4, 8) if "A" in fl else (4,) if "8" in fl else ()):
                    rows.append((f"{name} off {b}", {name: ("off", b)}))
            elif kind == "a":
                if "R" in fl or "r" in fl:
                    rows.append((f"null {name}[]", {name: None}))
                if "R" in fl:
                    rows.append((f"null {name}[{k}]", {name: ("null", k)}))
                for b in ((4, 8) if "A" in fl else ()):
                    rows.append((f"{name}[{k}] off {b}", {name: ("off", b, k)}))
        rows += [(f"{arg} short", {arg: "short"}) for arg in E.get("short", {})]
        for what, edits, *no_work in rows + list(E["rows"]):
            yield f"{entry}: {what}", entry, edits, bool(no_work and no_work[0])


def _desc(kind, name, v):
    cls, fields = DESC[kind]
    d = cls()
    for f in fields:
        x = v[f"{name}.{f}"]
        if isinstance(x, tuple):
            for i, e in enumerate(x):
                getattr(d, f)[i] = e
        else:
            setattr(d, f, x)
    return d


def call(lib, entry, edits):
    """the return code of `entry` for its valid call with `edits` applied"""
    E = ENTRIES[entry]
    v = _good(entry)
    v.update({n: e for n, e in edits.items() if n in v and e != "short"})
    descs, args, keep = {}, [], []
    for name, kind, *_ in E["params"]:
        if kind in DESC:
            descs[name] = ctypes.byref(_desc(kind, name, v))
    n_fill = v[E["n"]] if "n" in E else 0
    n_fill = _good(entry)[E["n"]] if "n" in E and not 0 <= n_fill <= NMAX else n_fill
    for j, (name, kind, *_) in enumerate(E["params"]):
        e = edits.get(name, "good")
        base = 4096 * (j + 1)
        if kind in DESC:
            args.append(None if e is None else descs[name])
        elif kind == "p":
            args.append(None if e is None else ctypes.c_void_p(base + (e[1] if isinstance(e, tuple) else 0)))
        elif kind == "h":
            keep.append(ctypes.create_string_buffer(4096))
            args.append(None if e is None else keep[-1])
        elif kind == "a":
            if e is None:
                args.append(None)
                continue
            a = (ctypes.c_void_p * 16)()
            for i in range(n_fill):
                a[i] = base + 64 * i
            if isinstance(e, tuple):
                a[e[-1]] = None if e[0] == "null" else base + 64 * e[-1] + e[1]
            keep.append(a)
            args.append(a)
        elif kind == "s":
            args.append(None)
        elif e == "short":
            args.append(E["short"][name](lib, v, descs) - 1)
        else:
            args.append(v[name])
    return getattr(lib, entry)(*args)


def gen(lib):
    reject = {}
    for key, entry, edits, no_work in reject_table():
        assert key not in reject, key
        code = call(lib, entry, edits)
        assert code != ERR_HIP and (code < 0 or no_work), (key, code)  # the row passed validation and reached a launch
        reject[key] = code
    return {"reject": reject}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libmtlora_hip.so to load instead of the tree's own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_rejects.json")
    with open(out, "w") as f:
        json.dump(gen(L.lib()), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
