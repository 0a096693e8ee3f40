#!/usr/bin/env python
"""Measure the device-side batch ingest (mtlora_amd/data.py, csrc/ingest.hip) at the shapes of a config (default c2: B = 32,
448 px, four PASCAL tasks).  HIP events, median of --steps after --warmup:

  (a) data.prepare_batch (one library call) against data.prepare_batch_torch (the ATen sequence) on the same GPU, with the
      bytes both move (wire format read + fp32 tensors written) over the kernel's time against the 6.29 TB/s copy ceiling;
  (b) the pinned host-to-device copy of one batch in wire format against the same batch as fp32 tensors;
  (c) img/s of --train-steps train steps fed by data.DeviceLoader from a pre-generated ring of host batches against the
      same steps on tensors that already live on the device, in one process, the legs alternating over --rounds.  The fed
      leg runs twice: from pageable host batches (staged through the loader's pinned ring) and from pinned ones (what a
      DataLoader with pin_memory=True yields; copied from where they are).

    python tools/bench_ingest.py [--config c2] [--batch 32] [--steps 10] [--warmup 3] [--train-steps 30] [--rounds 2]
                                 [--out profiles/ingest_bench_c2.json]

Prints one JSON line and writes it to --out.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mtlora_amd import data as D  # noqa: E402
from mtlora_amd import mtl_harness as H  # noqa: E402

COPY_CEILING = 6.29e12  # bytes / s, the copy ceiling the project quotes for the MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=30)
    ap.add_argument("--train-warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ring", type=int, default=4, help="pre-generated host batches the fed legs cycle through")
    ap.add_argument("--out", default=os.path.join("profiles", "ingest_bench_c2.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: needs a GPU (there is no CPU path to time)")
    cfg = H.config(a.config)
    tasks, S = list(cfg["tasks"]), cfg["img_size"]
    B = a.batch or cfg["batch"]
    dev = torch.device("cuda:0")
    res = {"config": a.config, "batch": B, "img_size": S, "tasks": tasks, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}

    # (a) the ingest alone
    host = [D.synthetic_wire_batch(B, S, tasks, seed=10 + i) for i in range(a.ring)]
    flip = (torch.rand(B, generator=torch.Generator().manual_seed(0)) < 0.5).to(torch.uint8)
    on_dev = {k: v.to(dev) for k, v in {**host[0], "flip": flip}.items()}
    img, tg = D.prepare_batch(on_dev, tasks)
    ref_img, ref_tg = D.prepare_batch_torch(on_dev, tasks)
    assert torch.equal(img, ref_img) and all(torch.equal(tg[t], ref_tg[t]) for t in tasks), "prepare_batch != prepare_batch_torch"
    moved = nbytes([on_dev[k] for k in ["image"] + tasks]) + nbytes([img] + list(tg.values()))
    hip_ms, hip_min = timed(lambda: D.prepare_batch(on_dev, tasks), a.steps, a.warmup)
    aten_ms, aten_min = timed(lambda: D.prepare_batch_torch(on_dev, tasks), a.steps, a.warmup)
    res["a_prepare_batch"] = {"hip_ms": hip_ms, "hip_ms_min": hip_min, "aten_ms": aten_ms, "aten_ms_min": aten_min,
                              "speedup": aten_ms / hip_ms, "bytes_read_plus_written": moved,
                              "hip_TBps": moved / (hip_ms * 1e-3) / 1e12,
                              "hip_share_of_copy_ceiling": moved / (hip_ms * 1e-3) / COPY_CEILING}

    # (b) pinned host-to-device copies: wire format against fp32 tensors
    wire_pinned = {k: v.pin_memory() for k, v in host[0].items()}
    cpu_img, cpu_tg = D.prepare_batch_torch(host[0], tasks)
    f32_pinned = [cpu_img.pin_memory()] + [cpu_tg[t].pin_memory() for t in tasks]
    wire_dst = {k: torch.empty_like(v, device=dev) for k, v in wire_pinned.items()}
    f32_dst = [torch.empty_like(v, device=dev) for v in f32_pinned]

    def h2d_wire():
        for k, v in wire_pinned.items():
            wire_dst[k].copy_(v, non_blocking=True)

    def h2d_f32():
        for d, v in zip(f32_dst, f32_pinned):
            d.copy_(v, non_blocking=True)

    w_ms, _ = timed(h2d_wire, a.steps, a.warmup)
    f_ms, _ = timed(h2d_f32, a.steps, a.warmup)
    wb, fb = nbytes(wire_pinned.values()), nbytes(f32_pinned)
    res["b_h2d_pinned"] = {"wire_ms": w_ms, "wire_bytes": wb, "wire_GBps": wb / (w_ms * 1e-3) / 1e9, "fp32_ms": f_ms,
                           "fp32_bytes": fb, "fp32_GBps": fb / (f_ms * 1e-3) / 1e9, "wire_MB_per_image": wb / B / 1e6,
                           "fp32_MB_per_image": fb / B / 1e6}
    del wire_dst, f32_dst, f32_pinned, cpu_img, cpu_tg, img, tg, ref_img, ref_tg

    # (c) train steps: resident tensors against DeviceLoader
    model = H.build_config_model(a.config, tasks=tasks).to(dev).train()
    crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model)
    resident = [tuple(D.prepare_batch({k: v.to(dev) for k, v in hb.items()}, tasks)) for hb in host]
    pinned = [{k: v.pin_memory() for k, v in hb.items()} for hb in host]
    n_w, n_t = a.train_warmup, a.train_steps

    def run(batches):
        it = iter(batches)
        for _ in range(n_w):
            H.train_step(model, crit, opt, *next(it))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_t):
            H.train_step(model, crit, opt, *next(it))
        torch.cuda.synchronize()
        return B * n_t / (time.perf_counter() - t0)

    def fed(ring):
        return D.DeviceLoader(itertools.islice(itertools.cycle(ring), n_w + n_t), tasks, dev, flip_p=0.5, seed=1, depth=2)

    legs = {"resident": [], "fed_pageable": [], "fed_pinned": []}
    for _ in range(a.rounds):
        legs["resident"].append(run(itertools.cycle(resident)))
        legs["fed_pageable"].append(run(fed(host)))
        legs["fed_pinned"].append(run(fed(pinned)))
    best = {k: max(v) for k, v in legs.items()}
    res["c_train_steps"] = {"train_steps": n_t, "train_warmup": n_w, "rounds": a.rounds, "img_per_s_runs": legs,
                            "img_per_s": best, "fed_pageable_over_resident": best["fed_pageable"] / best["resident"],
                            "fed_pinned_over_resident": best["fed_pinned"] / best["resident"], "acceptance": 0.98}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
