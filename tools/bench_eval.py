#!/usr/bin/env python
"""Time one validation batch of the c2 model (Swin-T 448, four PASCAL tasks, B = 32, bf16 autocast) two ways:

  fused      mtl_harness.validate_step: model(x, upsample=False), one metrics launch per task (csrc/metrics.hip)
  full-res   what the package offered before: model(x) writes the full-resolution predictions, then get_output and the
             torch meters + the plain losses on the same GPU

and, per task, the tail alone on that task's low-resolution head output (fused: the metrics launch with its label statistic;
full-res: interpolate + get_output + meter.update + task_loss).  HIP events after warm-up, median of --steps.

    python tools/bench_eval.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--tasks a,b,..] [--out FILE]

    python tools/bench_eval.py --masked [--batch 32] [--steps 10] [--warmup 3] [--inner 20] [--out FILE]

--masked times, instead, `functional.upsample_metrics` alone (label statistic + the k_up_metrics launch + the sum of its partials)
per task on synthetic bf16 head outputs at the heads' geometry (B x 56 x 56 at scale 8): the unmasked call, `valid=` with every
sample labelled and `valid=` with every second sample labelled.  Each timed window is --inner calls between two HIP events; the
three variants alternate inside every one of the --steps rounds, and the median, the minimum and the maximum per call are reported.

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


MASKED_TASKS = ("semseg", "human_parts", "normals", "sal", "depth", "edge")


def masked(a):
    """the partially labelled launch next to the unmasked one, per task, at the heads' geometry"""
    from mtlora_amd import functional as Fn
    from mtlora_amd.evaluation import FUSED_KIND
    dev = torch.device("cuda:0")
    B, h, w, S = a.batch or 32, 56, 56, 8
    tasks = tuple(a.tasks.split(",")) if a.tasks else MASKED_TASKS
    _, tg = H.synthetic_batch(B, h * S, tasks, seed=1, device=dev)
    g = torch.Generator().manual_seed(2)
    flags = {"unmasked": None, "valid_all": torch.ones(B, dtype=torch.uint8, device=dev),
             "valid_half": (torch.arange(B) % 2 == 0).to(torch.uint8).to(dev)}
    res = {"mode": "masked", "batch": B, "h": h, "w": w, "scale": S, "dtype": "bf16", "steps": a.steps, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "per_task_us": {}}
    for t in tasks:
        kind = FUSED_KIND[t]
        low = torch.randn(B, h, w, H.num_output(t), generator=g).to(dev).to(torch.bfloat16)
        ni, _ = Fn.upsample_metrics_sizes(kind, B, h, w, low.shape[-1], S)
        counts = torch.zeros(max(ni, 1), dtype=torch.int64, device=dev)

        def run(v):
            for _ in range(a.inner):
                Fn.upsample_metrics(kind, low, tg[t], S, counts=counts, valid=v)

        for v in flags.values():
            for _ in range(a.warmup):
                run(v)
        torch.cuda.synchronize()
        us = {k: [] for k in flags}
        for _ in range(a.steps):
            for k, v in flags.items():  # alternating: a drift of the machine hits the three alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(v)
                e1.record()
                torch.cuda.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.inner)
        res["per_task_us"][t] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in us.items()}
    return res


def emit(res, out):
    line = json.dumps(res)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tasks", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--masked", action="store_true", help="time upsample_metrics with and without valid= at the heads' geometry")
    ap.add_argument("--inner", type=int, default=20, help="--masked: calls per timed window")
    a = ap.parse_args()
    if a.masked:
        emit(masked(a), a.out)
        return
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
    emit(res, a.out)


if __name__ == "__main__":
    main()
