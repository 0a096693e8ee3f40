#!/usr/bin/env python3
"""Rank-aware dense update: one layer's Delta W formation, forward + backward, at the stage-0 and stage-1 shapes of c5:256.

    python tools/bench_delta.py [--iters 50] [--warmup 10] [--n 9] [--rank 256] [--shapes 288x96,96x96,...]

Times what ``lora._delta_factors`` does for the n = 1 + T updates of a layer (Delta W_i = s_i B_i A_i, then dA_i and dB_i from the
N x K gradients Z_i the linear backward returns) on both paths of this build: "hip", the ``Fn.DeltaFn`` launches
(``mtlora_delta_fwd`` / ``_bwd``, one each way), and "aten", the stack / bmm / mul / unbind sequence with its autograd backward
(``MTLORA_DELTA_HIP=0``).  A build without the HIP path (an older commit) times "aten" only.  Per shape: the median over --iters of
the HIP-event span of one forward + backward, and the host time per call of a back-to-back loop (the step is host-bound: the
number of launches is what this path costs)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import lora  # noqa: E402

SHAPES = "288x96,96x96,384x96,96x384,576x192,192x192,768x192,192x768"  # N x K of qkv, proj, fc1, fc2 at embed 96 and 192


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) / iters
    torch.cuda.synchronize()
    return statistics.median(ts) * 1e3, host * 1e6


def bench(N, K, n, r, iters, warm):
    As = [torch.randn(r, K, device="cuda").requires_grad_(True) for _ in range(n)]
    Bs = [torch.randn(N, r, device="cuda").requires_grad_(True) for _ in range(n)]
    Zs = [torch.randn(N, K, device="cuda") for _ in range(n)]
    scales = [2.0] + [1.5] * (n - 1)

    def step():
        ea, eb = lora._delta_factors(As, Bs, scales, K, N)
        torch.autograd.backward(eb if K <= N else ea, Zs)
        for p in As + Bs:
            p.grad = None

    out = {}
    paths = ["hip", "aten"] if hasattr(lora, "DELTA_HIP") else ["aten"]
    for path in paths:
        if len(paths) > 1:
            lora.DELTA_HIP = path == "hip"
        out[path] = timed(step, iters, warm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=9)
    ap.add_argument("--rank", type=int, default=256)
    ap.add_argument("--shapes", default=SHAPES)
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}  Delta W forward + backward of one layer, n = {a.n}, r = {a.rank}, median of {a.iters}: "
          "HIP-event span (us) / host time per call (us)")
    print(f"{'N':>6}{'K':>6}{'hip span':>10}{'hip host':>10}{'aten span':>11}{'aten host':>11}{'span x':>8}{'host x':>8}")
    for t in a.shapes.split(","):
        N, K = (int(v) for v in t.split("x"))
        res = bench(N, K, a.n, a.rank, a.iters, a.warmup)
        at = res["aten"]
        if "hip" in res:
            h = res["hip"]
            print(f"{N:>6}{K:>6}{h[0]:>10.1f}{h[1]:>10.1f}{at[0]:>11.1f}{at[1]:>11.1f}{at[0] / h[0]:>8.2f}{at[1] / h[1]:>8.2f}", flush=True)
        else:
            print(f"{N:>6}{K:>6}{'-':>10}{'-':>10}{at[0]:>11.1f}{at[1]:>11.1f}{'-':>8}{'-':>8}", flush=True)


if __name__ == "__main__":
    main()
