#!/usr/bin/env python
"""Time one validation batch of the c2 model (Swin-T 448, four PASCAL tasks, B = 32, bf16 autocast) two ways:

  fused      mtl_harness.validate_step: model(x, upsample=False), one metrics launch per task (csrc/metrics.hip)
  full-res   what the package offered before: model(x) writes the full-resolution predictions, then get_output and the
             torch meters + the plain losses on the same GPU

and, per task, the tail alone on that task's low-resolution head output (fused: the metrics launch with its label statistic;
full-res: interpolate + get_output + meter.update + task_loss).  HIP events after warm-up, median of --steps.

    python tools/bench_eval.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--tasks a,b,..] [--out FILE]

Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --steps 3` the k_up_metrics
launches appear next to everything else.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mtlora_amd import mtl_harness as H  # noqa: E402
from mtlora_amd.evaluation import PerformanceMeter, get_output  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tasks", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    cfg = H.config(a.config)
    tasks = tuple(a.tasks.split(",")) if a.tasks else cfg["tasks"]
    B = a.batch or cfg["batch"]
    dev = torch.device("cuda:0")
    model = H.build_config_model(a.config, tasks=tasks).to(dev).eval()
    crit = H.MultiTaskLoss(tasks)
    img, tg = H.synthetic_batch(B, cfg["img_size"], tasks, seed=1, device=dev)
    fused_meter, plain_meter = PerformanceMeter(tasks), PerformanceMeter(tasks)

    def fused():
        return H.validate_step(model, crit, fused_meter, img, tg)

    def full():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(img)
        with torch.no_grad():
            plain_meter.update({t: get_output(out[t].float(), t) for t in tasks}, tg)
            return crit(out, tg)

    res = {"config": a.config, "batch": B, "tasks": list(tasks), "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    res["fused_ms"], res["fused_min_ms"] = timed(fused, a.steps, a.warmup)
    fused_meter.reset()
    res["fullres_ms"], res["fullres_min_ms"] = timed(full, a.steps, a.warmup)
    plain_meter.reset()
    res["speedup"] = res["fullres_ms"] / res["fused_ms"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        low = model(img, upsample=False)
    per = {}
    for t in tasks:
        lo = low[t]

        def tail_fused():
            return fused_meter.update_task_low(t, lo, tg[t])

        def tail_full():
            with torch.no_grad():
                up = F.interpolate(lo.permute(0, 3, 1, 2), tg[t].shape[-2:], mode="bilinear")
                plain_meter.meters[t].update(get_output(up.float(), t), tg[t])
                return H.task_loss(t, up, tg[t])

        f, _ = timed(tail_fused, a.steps, a.warmup)
        p, _ = timed(tail_full, a.steps, a.warmup)
        per[t] = {"fused_tail_ms": f, "fullres_tail_ms": p}
        fused_meter.reset()
        plain_meter.reset()
    res["per_task"] = per
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
