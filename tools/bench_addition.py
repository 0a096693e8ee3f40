#!/usr/bin/env python3
"""SHARED_MODE "addition": the fused call (``functional.SumNormAddFn``: mtlora_sum_ln_add_fwd / _bwd) against the portable
torch definition (``functional.sum_norm_add_torch``) on the same tensors.

    python tools/bench_addition.py [--iters 30] [--out profiles/addition_ab.json]

Shapes: the four task-enabled ``fc1`` outputs of the c2 configuration (Swin-T / 448, batch 32): M = 32 * {112, 56, 28, 14}^2 rows,
N = 4C columns, T = 4 task outputs, bf16.  One iteration is a forward plus a backward in which ``out`` and every task output
receive a gradient (the task outputs feed the next layer as well, so the backward has its addends).  The two versions alternate
inside one process; each iteration is timed by device events; medians over --iters iterations after a warm-up of both.

bytes: what the algorithm has to move, counted in whole (M, N) 16-bit tensors and DERIVED from the shapes, not measured --
forward T + 2 (T task outputs and y in, out out), backward 3T + 1 (dout, T task outputs and T addends in, T gradients out).
``derived_gbps`` is that count over the measured time.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import functional as Fn  # noqa: E402

SHAPES = [(32 * s * s, 4 * c) for s, c in ((112, 96), (56, 192), (28, 384), (14, 768))]
T = 4


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def bench(M, N, iters, warm=5):
    dt = torch.bfloat16
    y = torch.randn(M, N, device="cuda", dtype=dt).requires_grad_(True)
    yts = [torch.randn(M, N, device="cuda", dtype=dt).requires_grad_(True) for _ in range(T)]
    norm = torch.nn.LayerNorm(N).cuda()
    gs = [torch.randn(M, N, device="cuda", dtype=dt) for _ in range(1 + T)]
    leaves = [y, *yts, norm.weight, norm.bias]
    assert Fn.sum_norm_add_ok(norm, y, yts)

    def clear():
        for q in leaves:
            q.grad = None

    def fused():
        clear()
        outs = Fn.SumNormAddFn.apply(y, norm.weight, norm.bias, norm.eps, *yts)
        torch.autograd.backward(outs, gs)

    def aten():
        clear()
        out = Fn.sum_norm_add_torch(y, yts, norm.weight, norm.bias, norm.eps)
        torch.autograd.backward([out, *yts], gs)

    # same result first (tolerance of a 16-bit output: 2^-8 of the largest value)
    fused()
    got = [q.grad.float().clone() for q in yts]
    aten()
    for a, b in zip(got, [q.grad.float() for q in yts]):
        assert ((a - b).abs().max() / b.abs().max()).item() < 2 ** -7
    for _ in range(warm):
        fused()
        aten()
    torch.cuda.synchronize()
    tf, ta = [], []
    for _ in range(iters):
        tf.append(one(fused))
        ta.append(one(aten))
    clear()
    return statistics.median(tf), statistics.median(ta), (min(tf), max(tf)), (min(ta), max(ta))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "addition_ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_addition: needs a GPU (a timing taken elsewhere says nothing about the kernels)")
    rows = []
    print(f"# {torch.cuda.get_device_name(0)}  bf16  T = {T}  fwd + bwd per iteration, median of {a.iters} (us)")
    print(f"{'M':>8}{'N':>6}{'fused':>10}{'torch':>10}{'torch/fused':>13}{'derived GB/s':>14}")
    for M, N in SHAPES:
        f, t, fr, tr = bench(M, N, a.iters)
        units = (T + 2) + (3 * T + 1)
        nbytes = units * M * N * 2
        rows.append({"M": M, "N": N, "T": T, "dtype": "bf16", "fused_us": f, "fused_us_min_max": fr, "torch_us": t, "torch_us_min_max": tr,
                     "torch_over_fused": t / f, "derived_units": units, "derived_bytes": nbytes, "derived_gbps": nbytes / f / 1e3})
        print(f"{M:>8}{N:>6}{f:>10.1f}{t:>10.1f}{t / f:>13.2f}{nbytes / f / 1e3:>14.0f}", flush=True)
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "what": "forward + backward, median us; bytes derived from shapes",
           "rows": rows, "fused_faster_everywhere": all(r["fused_us"] < r["torch_us"] for r in rows)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
