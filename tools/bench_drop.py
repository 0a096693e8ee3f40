#!/usr/bin/env python3
"""Activation dropout (MODEL.DROP_RATE) kernels against the ATen sequence they replace, and the c2 train step at drop_rate = 0.1.

    python tools/bench_drop.py [--iters 30] [--no-step] [--batch 32] [--steps 8]

(a) ``mtlora_act_dropout_fwd / _bwd`` (GELU + dropout of the 1+T hidden tensors, one launch per direction) against
    F.gelu + F.dropout and their backward per tensor;
(b) ``mtlora_residual_droppath_drop_fwd / _bwd`` (residual + DropPath + dropout of the 1+T branches) against F.dropout per branch
    followed by the plain residual kernels;
both in bf16 at the four c2 stage shapes (Swin-T / 448, batch 32), T = 0 and T = 4, forward + backward per iteration, with a plain
copy of the same bytes as the ceiling.  The train step runs through mtl_harness twice in one process: on the HIP path and with
``functional.act_dropout_ok`` answering no, which is the nn.Dropout path every call site falls back to (the code before the kernels).
Medians over --iters timed iterations after warm-up, HIP events around each iteration."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import _lib as L  # noqa: E402
from mtlora_amd import functional as Fn  # noqa: E402

STAGES = [(401408, 96), (100352, 192), (25088, 384), (6272, 768)]  # (rows, channels) of the c2 stages


def timed(fn, iters, warm=5):
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
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def copy_us(nbytes, iters):
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")  # a copy of n bytes moves n / 2 in and n / 2 out
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), iters)


def bench_act(M, C, n, p, iters):
    hs = [torch.randn(M, C, device="cuda", dtype=torch.bfloat16).requires_grad_(True) for _ in range(n)]
    gs = [torch.randn(M, C, device="cuda", dtype=torch.bfloat16) for _ in range(n)]

    def hip():
        outs = Fn.ActDropoutFn.apply(L.ACT_DROP_HIDDEN, L.ACT_GELU, p, 1234, *hs)
        torch.autograd.backward(outs, gs)

    def aten():
        outs = [torch.nn.functional.dropout(torch.nn.functional.gelu(h), p, True) for h in hs]
        torch.autograd.backward(outs, gs)

    t_hip, t_aten = timed(hip, iters), timed(aten, iters)
    for h in hs:
        h.grad = None
    nbytes = n * M * C * 2 * (2 + 3)  # forward: h in, a out; backward: g, h in, dh out
    return t_hip, t_aten, copy_us(nbytes, iters)


def bench_res(M, C, n, p, iters, B=32):
    res = torch.randn(B, M // B, C, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    ys = [torch.randn(B, M // B, C, device="cuda", dtype=torch.bfloat16).requires_grad_(True) for _ in range(n)]
    gs = [torch.randn(B, M // B, C, device="cuda", dtype=torch.bfloat16) for _ in range(n)]
    scale = (torch.rand(n, B, device="cuda") < 0.9).float() / 0.9

    def hip():
        outs = Fn.ResidualDropPathFn.apply(scale, True, n, res, *ys, p, 1234, L.ACT_DROP_PROJ)
        torch.autograd.backward(outs, gs)

    def aten():
        outs = Fn.ResidualDropPathFn.apply(scale, True, n, res, *[torch.nn.functional.dropout(y, p, True) for y in ys])
        torch.autograd.backward(outs, gs)

    t_hip, t_aten = timed(hip, iters), timed(aten, iters)
    nbytes = M * C * 2 * ((1 + 2 * n) + (2 * n + 1))  # forward: res + y_k in, out_k; backward: g_k in, dy_k + dres out
    return t_hip, t_aten, copy_us(nbytes, iters)


def bench_step(batch, steps, drop):
    from mtlora_amd import mtl_harness as H
    tasks = ("semseg", "normals", "sal", "human_parts")
    out = {}
    for label, ok in (("hip", None), ("aten", lambda ts: False)):
        model = H.build_model(img_size=448, tasks=tasks, seed=0).cuda().train()
        for m in model.modules():  # (build_model builds the shipped configs, drop_rate 0: set the rate where the constructor puts it)
            if isinstance(m, torch.nn.Dropout):
                m.p = drop
        img, tg = H.synthetic_batch(batch, 448, tasks, seed=1, device="cuda")
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model)
        keep = Fn.act_dropout_ok
        if ok is not None:
            Fn.act_dropout_ok = ok
        try:
            ms = timed(lambda: H.train_step(model, crit, opt, img, tg), steps, warm=3) / 1e3
        finally:
            Fn.act_dropout_ok = keep
        out[label] = ms
        del model, opt
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--p", type=float, default=0.1)
    a = ap.parse_args()
    print(f"# {torch.cuda.get_device_name(0)}  bf16  p = {a.p}  fwd + bwd per iteration, median of {a.iters} (us)")
    print(f"{'kernel':<10}{'rows':>8}{'C':>6}{'T':>3}{'hip':>10}{'aten':>10}{'copy':>10}{'aten/hip':>10}{'copy/hip':>10}")
    for name, fn, widen in (("act", bench_act, 4), ("residual", bench_res, 1)):
        for M, C in STAGES:
            for T in (0, 4):
                h, t, c = fn(M, C * widen, 1 + T, a.p, a.iters)
                print(f"{name:<10}{M:>8}{C * widen:>6}{T:>3}{h:>10.1f}{t:>10.1f}{c:>10.1f}{t / h:>10.2f}{c / h:>10.2f}", flush=True)
    if not a.no_step:
        r = bench_step(a.batch, a.steps, a.p)
        print(f"c2 train step, batch {a.batch}, drop_rate {a.p}: hip path {r['hip']:.1f} ms, nn.Dropout path {r['aten']:.1f} ms "
              f"({a.batch * 1e3 / r['hip']:.0f} vs {a.batch * 1e3 / r['aten']:.0f} img/s)")


if __name__ == "__main__":
    main()
