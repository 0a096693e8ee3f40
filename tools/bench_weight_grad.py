#!/usr/bin/env python3
"""Full fine-tuning (MODEL.MTLORA.FREEZE_PRETRAINED False: every `linear.weight` of the MTLoRALinear layers trains): the dense weight
gradient alone at the layer shapes of a configuration, and ms per train step of ``build_model(freeze=False)``.

    python tools/bench_weight_grad.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--iters 10] [--graph] [--no-kernel]
                                      [--no-step] [--tasks 0,4] [--shapes 401408x96x288x0,...]

The kernel part times ``mtlora_linear_weight_grad`` over 1 + T bf16 sources at the twelve layer shapes of the c2 backbone (qkv, proj,
fc1 and fc2 of the four stages at batch 32; T = 4 is the last block of a stage) against the ATen form it replaces (the fp32 sum G of
the sources, then ``G.t() @ x.float()``), with two yardsticks: a plain copy of the bytes the product has to read, and the bf16 MFMA
peak (2.5 PFLOP/s dense) for its 2 (1 + T) M N K flops.  A library without the entry (an older build) times the ATen form only.
The train step runs through mtl_harness with ``freeze=False``, eagerly (``train_step``) or, ``--graph``, as replays of a
``GraphedTrainStep`` with the capturable HIP AdamW; medians over --steps timed steps after warm-up, HIP events around each step, and
the peak allocated memory of the run."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import _lib as L  # noqa: E402

PEAK_BF16 = 2.5e15


def c2_shapes(batch=32, img=448, C=96):
    """(M, K, N) of qkv, proj, fc1, fc2 in the four stages"""
    out = []
    for s in range(4):
        c, m = C << s, batch * (img // 4 >> s) ** 2
        out += [(f"s{s}.qkv", m, c, 3 * c), (f"s{s}.proj", m, c, c), (f"s{s}.fc1", m, c, 4 * c), (f"s{s}.fc2", m, 4 * c, c)]
    return out


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


def bench_kernel(M, K, N, T, iters):
    lib = L.lib()
    x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
    gs = [torch.randn(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(1 + T)]
    hip_us = None
    if hasattr(lib, "mtlora_linear_weight_grad") and "mtlora_linear_weight_grad" in L.EXPORTS:
        d = L.LinearDesc()
        d.M, d.K, d.N, d.dtype, d.T = M, K, N, L.BF16, T
        sb = lib.mtlora_linear_weight_grad_scratch_bytes(ctypes.byref(d))
        scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
        dW = torch.empty(N, K, dtype=torch.float32, device="cuda")

        def hip():
            L.check(lib.mtlora_linear_weight_grad(ctypes.byref(d), L.ptr(x), L.ptr(gs[0]), L.ptr_array(gs[1:]), L.ptr(dW), L.ptr(scratch),
                                                  sb, L.stream_ptr()), "mtlora_linear_weight_grad")

        hip_us = timed(hip, iters) * 1e3

    def aten():
        G = gs[0].float()
        for g in gs[1:]:
            G = G + g.float()
        return G.t() @ x.float()

    aten_us = timed(aten, iters) * 1e3
    nbytes = ((1 + T) * M * N + M * K) * 2
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy of n bytes moves n / 2 in and n / 2 out
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src), iters) * 1e3
    return hip_us, aten_us, copy_us, 2.0 * (1 + T) * M * N * K


def bench_step(config, batch, steps, warmup, graph):
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    c = H.config(config)
    model = H.build_config_model(config, seed=0, freeze=False).cuda().train()
    tasks = list(model.tasks)
    img, tg = H.synthetic_batch(batch, c["img_size"], tasks, seed=1, device="cuda")
    crit = H.MultiTaskLoss(tasks)
    n_w = sum(1 for n, p in model.backbone.named_parameters() if n.endswith("linear.weight") and p.requires_grad)
    torch.cuda.reset_peak_memory_stats()
    try:
        if graph:
            opt = H.build_optimizer(model, impl="hip", capturable=True)
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, warmup=warmup)
            if not gs.graphed:
                return None, n_w, gs.why, 0
            ms = timed(gs, steps, warm=2)
        else:
            opt = H.build_optimizer(model)
            ms = timed(lambda: H.train_step(model, crit, opt, img, tg), steps, warm=warmup)
    finally:
        Fn.set_seed_offset(None)
    peak = torch.cuda.max_memory_allocated()
    del model, opt
    torch.cuda.empty_cache()
    return ms, n_w, "", peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--tasks", default="0,4", help="task counts T to time each shape with")
    ap.add_argument("--shapes", default="", help="M x K x N x T quadruples instead of the c2 table (a profiler run of one shape)")
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}  ABI v{L.lib().mtlora_version()}")
    if not a.no_kernel:
        print(f"# dense weight gradient, bf16 sources, median of {a.iters} (us); copy = the bytes read, moved by a plain copy; "
              f"peak = fraction of {PEAK_BF16 / 1e15:.1f} PFLOP/s")
        print(f"{'layer':>8}{'M':>8}{'K':>6}{'N':>6}{'T':>3}{'hip':>10}{'aten':>10}{'copy':>10}{'copy/hip':>10}{'peak':>8}{'aten/hip':>10}")
        if a.shapes:
            shapes = [("-",) + tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",")]
        else:
            shapes = [(n, M, K, N, int(T)) for n, M, K, N in c2_shapes(a.batch) for T in a.tasks.split(",")]
        for name, M, K, N, T in shapes:
            h, t, c, fl = bench_kernel(M, K, N, T, a.iters)
            if h is None:
                print(f"{name:>8}{M:>8}{K:>6}{N:>6}{T:>3}{'-':>10}{t:>10.1f}{c:>10.1f}{'-':>10}{'-':>8}{'-':>10}", flush=True)
            else:
                print(f"{name:>8}{M:>8}{K:>6}{N:>6}{T:>3}{h:>10.1f}{t:>10.1f}{c:>10.1f}{c / h:>10.2f}{fl / (h * 1e-6) / PEAK_BF16:>8.3f}"
                      f"{t / h:>10.2f}", flush=True)
    if not a.no_step:
        ms, n_w, why, peak = bench_step(a.config, a.batch, a.steps, a.warmup, a.graph)
        how = "graph replay" if a.graph else "eager"
        if ms is None:
            print(f"{a.config} batch {a.batch} freeze=False ({n_w} trainable linear weights), {how}: capture failed: {why}", flush=True)
        else:
            print(f"{a.config} batch {a.batch} freeze=False ({n_w} trainable linear weights), {how}: {ms:.2f} ms/step "
                  f"({a.batch * 1e3 / ms:.0f} img/s), peak allocated {peak / 2**30:.2f} GiB", flush=True)


if __name__ == "__main__":
    main()
