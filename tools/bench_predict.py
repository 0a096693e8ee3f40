#!/usr/bin/env python
"""Time the full-resolution predictions of one batch of the c2 model (Swin-T 448, four PASCAL tasks, B = 32, bf16 autocast):

  fused      mtl_harness.predict_step: model(x, upsample=False), one predict launch per task (csrc/predict.hip), with fp32
             and with uint8 images
  full-res   what the package offered before: model(x, upsample=True) writes the full-resolution logits, then get_output

and, per task, the predict launch alone on that task's low-resolution head output, with the bytes it writes over its time
against the 6.29 TB/s copy ceiling.  HIP events after warm-up, median of --steps (the launches alone: --reps back to back
inside one pair of events).

    python tools/bench_predict.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--reps 20] [--out profiles/predict_ab.txt]

Prints one JSON line and writes the table to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mtlora_amd import functional as Fn  # noqa: E402
from mtlora_amd import mtl_harness as H  # noqa: E402
from mtlora_amd.evaluation import PREDICT_KIND, get_output, get_output_low  # noqa: E402

COPY_CEILING = 6.29e12  # bytes / s, the copy ceiling the project quotes for the MI355X


def timed(fn, steps, warmup, reps=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "predict_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict: needs a GPU (there is no CPU path to time)")
    cfg = H.config(a.config)
    tasks = cfg["tasks"]
    B = a.batch or cfg["batch"]
    dev = torch.device("cuda:0")
    model = H.build_config_model(a.config, tasks=tasks).to(dev).eval()
    img, _ = H.synthetic_batch(B, cfg["img_size"], tasks, seed=1, device=dev)

    def full():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(img, upsample=True)
        with torch.no_grad():
            return {t: get_output(out[t], t) for t in tasks}

    res = {"config": a.config, "batch": B, "tasks": list(tasks), "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    # the two routes alternate, so that a drift of the box shows in both
    f32, u8, old = [], [], []
    for _ in range(2):
        f32.append(timed(lambda: H.predict_step(model, img), a.steps, a.warmup)[0])
        old.append(timed(full, a.steps, a.warmup)[0])
        u8.append(timed(lambda: H.predict_step(model, img, uint8=True), a.steps, a.warmup)[0])
    res["fused_fp32_ms"], res["fused_uint8_ms"], res["fullres_ms"] = min(f32), min(u8), min(old)
    res["fused_fp32_ms_runs"], res["fused_uint8_ms_runs"], res["fullres_ms_runs"] = f32, u8, old
    res["speedup_fp32"], res["speedup_uint8"] = res["fullres_ms"] / res["fused_fp32_ms"], res["fullres_ms"] / res["fused_uint8_ms"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        low = model(img, upsample=False)
    per = {}
    for t in tasks:
        lo = low[t]
        scale = cfg["img_size"] // lo.shape[1]
        forms = [False] if PREDICT_KIND[t] in ("argmax", "identity") else [False, True]
        for u in forms:
            out = get_output_low(lo, t, scale, uint8=u)
            ms, _ = timed(lambda: Fn.upsample_predict(PREDICT_KIND[t], lo, scale, out=out), a.steps, a.warmup, a.reps)
            nbytes = out.numel() * out.element_size()
            per[f"{t}:{str(out.dtype).replace('torch.', '')}"] = {
                "launch_ms": ms, "bytes_written": nbytes, "bytes_read": lo.numel() * lo.element_size(),
                "write_TBps": nbytes / (ms * 1e-3) / 1e12, "share_of_copy_ceiling": nbytes / (ms * 1e-3) / COPY_CEILING}
    res["launches"] = per
    line = json.dumps(res)
    lines = [f"# tools/bench_predict.py --config {a.config} --batch {B} --steps {a.steps} --warmup {a.warmup} --reps {a.reps}",
             f"# {res['device']}; ms per batch, median of {a.steps} after {a.warmup} warm-up, best of 2 alternating rounds",
             f"predict_step fp32 images   {res['fused_fp32_ms']:8.2f} ms   (rounds {', '.join(f'{v:.2f}' for v in f32)})",
             f"predict_step uint8 images  {res['fused_uint8_ms']:8.2f} ms   (rounds {', '.join(f'{v:.2f}' for v in u8)})",
             f"model(x) + get_output      {res['fullres_ms']:8.2f} ms   (rounds {', '.join(f'{v:.2f}' for v in old)})",
             f"speed-up                   {res['speedup_fp32']:8.2f} x fp32, {res['speedup_uint8']:.2f} x uint8",
             f"# the predict launches alone, into a given tensor ({a.reps} back to back between two events)",
             f"# {'task:out':<20s} {'ms':>8s} {'MB written':>11s} {'MB read':>9s} {'TB/s written':>13s} {'of 6.29 TB/s':>13s}"]
    for k, v in per.items():
        lines.append(f"  {k:<20s} {v['launch_ms']:8.4f} {v['bytes_written'] / 1e6:11.2f} {v['bytes_read'] / 1e6:9.2f} "
                     f"{v['write_TBps']:13.3f} {100 * v['share_of_copy_ceiling']:12.1f}%")
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
