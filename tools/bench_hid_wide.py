#!/usr/bin/env python3
"""Task-enabled Mlp at task ranks 16 .. 128: the implicit-task-hiddens path (``functional.set_mlp_hid_wide(True)``: csrc/hid_wide.h)
against the per-layer path (the default) on the same module and tensors.

    python tools/bench_hid_wide.py [--iters 20] [--out profiles/hid_wide_ab.json]

Shapes: the Mlp of c4 (Swin-B / 448, batch 16, 4 tasks, r = 128 shared and per task) at stages 0-3, and of c5:16 / c5:64 (Swin-T / 448,
batch 32, 8 tasks, r = 16 / 64) at stages 0 and 2; bf16 autocast.  Per shape: forward alone and forward + backward (every output
receives a gradient), the two paths alternating inside one process, each iteration timed by device events, medians over --iters
iterations after a warm-up of both.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import functional as Fn  # noqa: E402
from mtlora_amd import mtl_harness as H  # noqa: E402
from mtlora_amd.swin_transformer_mtlora import Mlp  # noqa: E402

# name: (M, C, tasks, rank)
SHAPES = {**{f"c4.s{i}": (16 * s * s, 128 << i, 4, 128) for i, s in enumerate((112, 56, 28, 14))},
          "c5:16.s0": (32 * 112 * 112, 96, 8, 16), "c5:16.s2": (32 * 28 * 28, 384, 8, 16),
          "c5:64.s0": (32 * 112 * 112, 96, 8, 64), "c5:64.s2": (32 * 28 * 28, 384, 8, 64)}


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def bench(M, C, T, r, iters, warm=3):
    tasks = [f"t{i}" for i in range(T)]
    torch.manual_seed(3)
    mlp = Mlp(C, 4 * C, lora=True, tasks=tasks, layer_idx=0, mtlora=H.mtlora_namespace(tasks, r_shared=r, r_task=r, scale=2.0, dropout=0.0)).cuda()
    with torch.no_grad():
        for n_, p_ in mlp.named_parameters():
            if "lora_" in n_:
                p_.normal_(0, 0.05)
            else:
                p_.requires_grad_(False)
    mlp.train()
    xs = [torch.randn(M, C, device="cuda", dtype=torch.bfloat16).requires_grad_(True) for _ in range(1 + T)]
    gs = [torch.randn(M, C, device="cuda", dtype=torch.bfloat16) for _ in range(1 + T)]

    def run(wide, backward):
        old = Fn.set_mlp_hid_wide(wide)
        try:
            for q in xs:
                q.grad = None
            mlp.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y, y_t = mlp(xs[0], dict(zip(tasks, xs[1:])))
            outs = [y] + [y_t[t] for t in tasks]
            if backward:
                torch.autograd.backward(outs, gs)
            return outs
        finally:
            Fn.set_mlp_hid_wide(old)

    # same result first (16-bit outputs of two roundings of the same sums)
    for a, b in zip(run(True, False), run(False, False)):
        assert ((a.float() - b.float()).abs().max() / b.float().abs().max()).item() < 2e-2
    res = {}
    for backward in (False, True):
        for _ in range(warm):
            run(True, backward)
            run(False, backward)
        torch.cuda.synchronize()
        tw, tl = [], []
        for _ in range(iters):
            tw.append(one(lambda: run(True, backward)))
            tl.append(one(lambda: run(False, backward)))
        k = "fwd_bwd" if backward else "fwd"
        res[k] = {"wide_us": statistics.median(tw), "wide_us_min_max": (min(tw), max(tw)), "per_layer_us": statistics.median(tl),
                  "per_layer_us_min_max": (min(tl), max(tl)), "per_layer_over_wide": statistics.median(tl) / statistics.median(tw)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hid_wide_ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hid_wide: needs a GPU (a timing taken elsewhere says nothing about the kernels)")
    print(f"# {torch.cuda.get_device_name(0)}  bf16  median of {a.iters} (us): implicit task hiddens (wide) vs per-layer path")
    print(f"{'shape':>10}{'M':>8}{'H':>6}{'T':>3}{'r':>5}{'fwd wide':>11}{'fwd layer':>11}{'ratio':>7}{'f+b wide':>11}{'f+b layer':>11}{'ratio':>7}")
    rows = []
    for name, (M, C, T, r) in SHAPES.items():
        res = bench(M, C, T, r, a.iters)
        rows.append({"shape": name, "M": M, "C": C, "H": 4 * C, "T": T, "r": r, "dtype": "bf16", **res})
        f, b = res["fwd"], res["fwd_bwd"]
        print(f"{name:>10}{M:>8}{4 * C:>6}{T:>3}{r:>5}{f['wide_us']:>11.0f}{f['per_layer_us']:>11.0f}{f['per_layer_over_wide']:>7.2f}"
              f"{b['wide_us']:>11.0f}{b['per_layer_us']:>11.0f}{b['per_layer_over_wide']:>7.2f}", flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "what": "Mlp forward / forward + backward, median us", "rows": rows},
                  fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
