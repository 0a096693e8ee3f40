#!/usr/bin/env python
"""Measure the device-side ScaleNRotate + FixedResize (mtlora_amd/data.py, csrc/augment.hip): B = 32 samples on a 500 x 500
canvas (PASCAL's largest side; sample sizes drawn in [250, 500]), 448 x 448 output, the four PASCAL tasks of c2, rotation in
(-20, 20) degrees and scale in (.75, 1.25).  HIP events, median of --steps after --warmup:

  data.augment_batch (one library call, one launch) against data.augment_batch_torch (the definition, as ATen ops) on the same
  GPU and the same batch, with the bytes the kernel writes (the wire-format batch) and the outputs of the two compared
  (uint8 outputs must be equal; the float outputs are reported as a largest distance in units in the last place, because
  ATen's division and square root on the device are not this project's to vouch for).

    python tools/bench_augment.py [--batch 32] [--canvas 500] [--out-size 448] [--steps 20] [--warmup 5] [--torch-steps 3]
                                  [--out profiles/augment_bench.json]

Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mtlora_amd import data as D  # noqa: E402

TASKS = ["semseg", "human_parts", "sal", "normals"]  # c2: the four PASCAL tasks


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


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts)


def ulps(a, b):
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return int((key(a) - key(b)).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--canvas", type=int, default=500)
    ap.add_argument("--out-size", type=int, default=448)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "augment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, S, O = a.batch, a.canvas, (a.out_size, a.out_size)
    raw = D.synthetic_raw_batch(B, S, S, TASKS, seed=10)
    g = torch.Generator().manual_seed(0)
    rot = 40.0 * torch.rand(B, generator=g, dtype=torch.float64) - 20.0
    sc = 0.5 * torch.rand(B, generator=g, dtype=torch.float64) + 0.75
    geom = D.make_geometry(raw["size"], rot, sc, O)
    on_dev = {k: v.to(dev) for k, v in raw.items()}
    dgeom = D.Geometry(geom.coef.to(dev), geom.side.to(dev))
    res = {"batch": B, "canvas": [S, S], "out_size": list(O), "tasks": TASKS, "steps": a.steps, "warmup": a.warmup,
           "torch_steps": a.torch_steps, "device": torch.cuda.get_device_name(0)}

    got = D.augment_batch(on_dev, TASKS, dgeom, O)
    ref = D.augment_batch_torch(on_dev, TASKS, dgeom, O)
    for k in ["image", "semseg", "human_parts", "sal"]:
        assert torch.equal(got[k], ref[k]), f"augment_batch != augment_batch_torch: {k}"
    stage = D.augment_batch(on_dev, ["normals"], dgeom, O, renormalize=False)["normals"]
    ref_stage = D.augment_batch_torch(on_dev, ["normals"], dgeom, O, renormalize=False)["normals"]
    res["normals_ulps_before_renorm_vs_aten_on_device"] = ulps(stage, ref_stage)
    res["normals_ulps_vs_aten_on_device"] = ulps(got["normals"], ref["normals"])
    written = nbytes([got[k] for k in ["image"] + TASKS])
    res["bytes_written"] = written
    res["bytes_raw_batch"] = nbytes([on_dev[k] for k in ["image"] + TASKS])
    del ref, ref_stage, stage

    hip_ms, hip_min = timed(lambda: D.augment_batch(on_dev, TASKS, dgeom, O), a.steps, a.warmup)
    aten_ms, aten_min = timed(lambda: D.augment_batch_torch(on_dev, TASKS, dgeom, O), a.torch_steps, 1)
    res.update({"hip_ms": hip_ms, "hip_ms_min": hip_min, "aten_ms": aten_ms, "aten_ms_min": aten_min, "speedup": aten_ms / hip_ms,
                "hip_written_GBps": written / (hip_ms * 1e-3) / 1e9, "hip_img_per_s": B / (hip_ms * 1e-3)})
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
