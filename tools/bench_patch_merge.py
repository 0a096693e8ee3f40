#!/usr/bin/env python
"""Time PatchMerging.forward_multi over the shared + task streams (bf16 autocast, fp32 residual streams, norm and reduction
trainable, streams wanting gradients) at the three stage boundaries of a backbone, on the same module and inputs, both ways,
alternating in one process:

  fused     swin_transformer_mtlora.PATCH_MERGE on: functional.PatchMergeFn, one launch forward, three backward (csrc/patch_merge.hip)
  separate  the switch off: the LayerNorm-merge launch over the streams, BigLinearFn (hipBLASLt forward and dX, batched dW + sum) and
            the LayerNorm backward launches

HIP events around --inner calls after warm-up, median of --steps windows, best of --rounds alternating rounds; next to each time the
host's time to ISSUE one call and the kernel launches of one call (torch.profiler, device-side kernel events).  Default shapes: c2
(Swin-T at 448 px, B = 32, 1 + 4 streams) and, with --dims 128, Swin-B.

    python tools/bench_patch_merge.py [--batch 32] [--streams 5] [--size 448] [--dims 96 128] [--out profiles/patch_merge_bench.txt]

Prints one JSON line per shape and writes the table to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--streams", type=int, default=5)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--dims", type=int, nargs="+", default=[96, 128])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "patch_merge_bench.txt"))
    a = ap.parse_args()
    import torch
    from mtlora_amd import swin_transformer_mtlora as S
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_patch_merge.py --batch {a.batch} --streams {a.streams} --size {a.size} --dims {' '.join(map(str, a.dims))} "
             f"--steps {a.steps} --warmup {a.warmup} --inner {a.inner} --rounds {a.rounds}",
             f"# {torch.cuda.get_device_name(0)}; bf16 autocast, fp32 streams; us per call by device events (host issue us) [kernel launches], "
             f"median of {a.steps} windows of {a.inner} calls, best of {a.rounds} alternating rounds",
             f"# {'shape (H x W, C)':<18s} {'pass':<8s} {'fused':>24s} {'separate':>24s} {'speed-up':>9s}"]
    prev = S.PATCH_MERGE
    try:
        for dim in a.dims:
            for stage in range(3):
                H, C = a.size // 4 >> stage, dim << stage
                torch.manual_seed(0)
                mod = S.PatchMerging((H, H), dim=C, mtlora=SimpleNamespace(DOWNSAMPLER_ENABLED=False)).to(dev)
                xs = [torch.randn(a.batch, H * H, C, device=dev).requires_grad_(True) for _ in range(a.streams)]
                gy = torch.randn(a.streams * a.batch, H * H // 4, 2 * C, device=dev, dtype=torch.bfloat16)

                def step(on, train):
                    S.PATCH_MERGE = on
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        if not train:
                            with torch.no_grad():
                                return torch.stack(mod.forward_multi(xs))
                        y = torch.stack(mod.forward_multi(xs))
                    mod.zero_grad(set_to_none=True)
                    for x in xs:
                        x.grad = None
                    y.flatten(0, 1).backward(gy)
                    return y

                def timed(on, train):
                    for _ in range(a.warmup):
                        step(on, train)
                    torch.cuda.synchronize()
                    ms, host = [], []
                    for _ in range(a.steps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        t0 = time.perf_counter()
                        for _ in range(a.inner):
                            step(on, train)
                        host.append((time.perf_counter() - t0) / a.inner)
                        e1.record()
                        torch.cuda.synchronize()
                        ms.append(e0.elapsed_time(e1) / a.inner)
                    return 1e3 * statistics.median(ms), 1e6 * statistics.median(host)

                def launches(on, train):
                    step(on, train)
                    torch.cuda.synchronize()
                    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                        step(on, train)
                        torch.cuda.synchronize()
                    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

                y1, g1 = step(True, True).float(), [t.grad.clone() for t in list(mod.parameters()) + xs]
                y0, g0 = step(False, True).float(), [t.grad.clone() for t in list(mod.parameters()) + xs]
                diff = {"y": ((y1 - y0).abs().max() / y0.abs().max()).item(),
                        "grads": max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(g1, g0))}
                keys = (("fused", True, True), ("separate", False, True), ("fused_fwd", True, False), ("separate_fwd", False, False))
                t, issue = {k: [] for k, _, _ in keys}, {k: [] for k, _, _ in keys}
                for _ in range(a.rounds):  # the routes alternate, so that a drift of the box shows in both
                    for k, on, train in keys:
                        us, host_us = timed(on, train)
                        t[k].append(us)
                        issue[k].append(host_us)
                n_k = {k: launches(on, train) for k, on, train in keys}
                best, host = {k: min(v) for k, v in t.items()}, {k: min(v) for k, v in issue.items()}
                res = {"batch": a.batch, "streams": a.streams, "H": H, "C": C, "rows": a.streams * a.batch * H * H // 4, "us": best,
                       "host_issue_us": host, "launches": n_k, "us_rounds": t, "rel_diff_fused_vs_separate": diff}
                for name, f, s in (("fwd+bwd", "fused", "separate"), ("fwd", "fused_fwd", "separate_fwd")):
                    cell = lambda k: f"{best[k]:10.1f} ({host[k]:7.1f}) [{n_k[k]:2d}]"  # noqa: E731
                    lines.append(f"  {f'{H} x {H}, {C}':<18s} {name:<8s} {cell(f):>24s} {cell(s):>24s} {best[s] / best[f]:9.2f}")
                lines.append(f"#   fused against separate, relative to max |separate|: y {diff['y']:.2e}, gradients {diff['grads']:.2e}")
                lines.append(json.dumps(res))
                del mod, xs, gy, y1, y0, g1, g0
                torch.cuda.empty_cache()
    finally:
        S.PATCH_MERGE = prev
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
