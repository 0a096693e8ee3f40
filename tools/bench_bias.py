#!/usr/bin/env python3
"""MODEL.MTLORA.BIAS 'all' (every `*.bias` of the backbone trains, the frozen linears' among them) against 'none': ms per train
step of a configuration, and the bias-gradient reduction alone against the ATen form it replaces.

    python tools/bench_bias.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--graph] [--modes none,all] [--no-kernel]
                               [--no-step] [--shapes 401408x384x4,...]

The train step runs through mtl_harness (``build_config_model(..., bias=mode)``), one mode after the other in one process, eagerly
(``train_step``, with the harness' side streams) or, ``--graph``, as replays of a ``GraphedTrainStep`` with the capturable HIP AdamW.
Medians over --steps timed steps after warm-up, HIP events around each step.  The kernel part times ``mtlora_linear_bias_grad``
over 1 + T bf16 sources at the c2 stage shapes of fc1 against ``sum_k g_k.float()`` followed by ``.sum(0)``, with a plain copy of the
bytes the reduction has to read as the ceiling."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import _lib as L  # noqa: E402

FC1 = [(401408, 384), (100352, 768), (25088, 1536), (6272, 3072)]  # (rows, hidden width) of fc1 in the four c2 stages


def timed(fn, iters, warm=3):
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
    return statistics.median(ts)


def bench_kernel(M, N, T, iters):
    lib = L.lib()
    gs = [torch.randn(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(1 + T)]
    d = L.LinearDesc()
    d.M, d.K, d.N, d.dtype, d.T = M, N, N, L.BF16, T
    sb = lib.mtlora_linear_bias_grad_scratch_bytes(ctypes.byref(d))
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    db = torch.empty(N, dtype=torch.float32, device="cuda")

    def hip():
        L.check(lib.mtlora_linear_bias_grad(ctypes.byref(d), L.ptr(gs[0]), L.ptr_array(gs[1:]), L.ptr(db), L.ptr(scratch), sb,
                                            L.stream_ptr()), "mtlora_linear_bias_grad")

    def aten():
        G = gs[0].float()
        for g in gs[1:]:
            G = G + g.float()
        return G.sum(0)

    nbytes = (1 + T) * M * N * 2
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy of n bytes moves n / 2 in and n / 2 out
    dst = torch.empty_like(src)
    return timed(hip, iters) * 1e3, timed(aten, iters) * 1e3, timed(lambda: dst.copy_(src), iters) * 1e3, nbytes


def bench_step(config, batch, steps, warmup, graph, mode):
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    c = H.config(config)
    model = H.build_config_model(config, seed=0, bias=mode).cuda().train()
    tasks = list(model.tasks)
    img, tg = H.synthetic_batch(batch, c["img_size"], tasks, seed=1, device="cuda")
    crit = H.MultiTaskLoss(tasks)
    n_bias = sum(1 for n, p in model.backbone.named_parameters() if n.endswith("linear.bias") and p.requires_grad)
    try:
        if graph:
            opt = H.build_optimizer(model, impl="hip", capturable=True)
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, warmup=warmup)
            if not gs.graphed:
                return None, n_bias, gs.why
            ms = timed(gs, steps, warm=2)
        else:
            opt = H.build_optimizer(model)
            ms = timed(lambda: H.train_step(model, crit, opt, img, tg), steps, warm=warmup)
    finally:
        Fn.set_seed_offset(None)
    del model, opt
    torch.cuda.empty_cache()
    return ms, n_bias, ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--modes", default="none,all")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--shapes", default="", help="rows x width x T triples instead of the c2 fc1 table (a profiler run of one shape)")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}  ABI v{L.lib().mtlora_version()}")
    if not a.no_kernel:
        print(f"# mtlora_linear_bias_grad, bf16 sources, median of {a.iters} (us); copy = the same bytes moved by a plain copy")
        print(f"{'rows':>8}{'N':>6}{'T':>3}{'hip':>10}{'aten':>10}{'copy':>10}{'TB/s':>8}{'aten/hip':>10}")
        shapes = ([tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",")] if a.shapes
                  else [(M, N, T) for M, N in FC1 for T in (0, 4)])
        for M, N, T in shapes:
            h, t, c, nb = bench_kernel(M, N, T, a.iters)
            print(f"{M:>8}{N:>6}{T:>3}{h:>10.1f}{t:>10.1f}{c:>10.1f}{nb / h / 1e6:>8.2f}{t / h:>10.2f}", flush=True)
    if not a.no_step:
        for mode in a.modes.split(","):
            ms, n_bias, why = bench_step(a.config, a.batch, a.steps, a.warmup, a.graph, mode)
            how = "graph replay" if a.graph else "eager"
            if ms is None:
                print(f"{a.config} batch {a.batch} bias={mode} ({n_bias} trainable linear biases), {how}: capture failed: {why}", flush=True)
            else:
                print(f"{a.config} batch {a.batch} bias={mode} ({n_bias} trainable linear biases), {how}: {ms:.2f} ms/step "
                      f"({a.batch * 1e3 / ms:.0f} img/s)", flush=True)


if __name__ == "__main__":
    main()
