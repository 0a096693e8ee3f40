#!/usr/bin/env python3
"""The c2 train step (Swin-T / 448, four tasks, r 64 / 4, batch 32, bf16) with TRAINABLE_SCALE_SHARED and TRAINABLE_SCALE_PER_TASK on.

    python tools/bench_trainable_scale.py [--batch 32] [--steps 10] [--repeats 3] [--graph]

Per repeat: a fresh model, 3 warm-up steps, then --steps timed steps of ``mtl_harness.train_step`` (or of a ``GraphedTrainStep``
replay with --graph, FusedAdamW(capturable=True)).  Prints ms/step (HIP events around the timed block) and the host-issue time
(wall time of the Python calls that issue one step, before any wait), median over the repeats with the range.  Uses nothing but
mtl_harness, so the same file measures a commit from before the scales lived on the device (where --graph cannot capture)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import functional as Fn  # noqa: E402
from mtlora_amd import mtl_harness as H  # noqa: E402

TASKS = ("semseg", "normals", "sal", "human_parts")


def one(batch, steps, graph, flags):
    model = H.build_model(img_size=448, tasks=TASKS, seed=0, **flags).cuda().train()
    img, tg = H.synthetic_batch(batch, 448, TASKS, seed=1, device="cuda")
    crit = H.MultiTaskLoss(TASKS)
    if graph:
        opt = H.build_optimizer(model, impl="hip", capturable=True)
        gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=3)
        if not gs.graphed:
            raise RuntimeError("capture failed: " + gs.why)
        step = gs
    else:
        opt = H.build_optimizer(model)
        step = lambda: H.train_step(model, crit, opt, img, tg)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = []
    a.record()
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        host.append((time.perf_counter() - t0) * 1e3)
    b.record()
    b.synchronize()
    Fn.set_seed_offset(None)
    return a.elapsed_time(b) / steps, statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--constant", action="store_true", help="the same step with constant scales (the shipped c2)")
    a = ap.parse_args()
    flags = {} if a.constant else dict(TRAINABLE_SCALE_SHARED=True, TRAINABLE_SCALE_PER_TASK=True)
    runs = []
    for _ in range(a.repeats):
        runs.append(one(a.batch, a.steps, a.graph, flags))
        torch.cuda.empty_cache()
    ms, host = [r[0] for r in runs], [r[1] for r in runs]
    print(f"# {torch.cuda.get_device_name(0)}  c2 batch {a.batch}  {'graph replay' if a.graph else 'eager'}  "
          f"{'constant scales' if a.constant else 'trainable scales'}  {a.repeats} x {a.steps} steps")
    print(f"ms/step {statistics.median(ms):.2f} ({min(ms):.2f} .. {max(ms):.2f})   host issue ms/step {statistics.median(host):.2f} "
          f"({min(host):.2f} .. {max(host):.2f})   {a.batch * 1e3 / statistics.median(ms):.0f} img/s")


if __name__ == "__main__":
    main()
