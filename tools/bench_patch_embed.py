#!/usr/bin/env python
"""Time the patch embedding of the c2 model (B = 32, 3 x 448 x 448, E = 96, bf16 autocast: M = 401 408 tokens), forward +
backward with proj and norm trainable, on the same module and image, both ways, alternating in one process:

  fused     swin_transformer_mtlora.PATCH_EMBED on: functional.PatchEmbedFn, one launch forward, two backward (csrc/patch_embed.hip)
  separate  the switch off: ATen gather of the (M, 48) patch matrix, cast, BigLinearFn, LayerNormFn and their backward launches

HIP events around --inner forward + backward pairs after warm-up (windows of tens of milliseconds), median of --steps windows, best
of --rounds alternating rounds; the rate is the bytes the algorithm must move (image once each way, tokens out, token gradient in)
over the fused time.  The forward alone (under no_grad) is timed the same way.  These are times per call as a training loop sees
them, not kernel times: next to each the tool prints the host's time to ISSUE one call (host clock around the window's loop, before
the synchronise).  Where the issue time is below the event time the GPU is the bound; where the two are equal the route is bound by
the host's launches, and a captured graph would run it faster than the figure says.

    python tools/bench_patch_embed.py [--batch 32] [--size 448] [--steps 10] [--warmup 3] [--inner 100] [--rounds 3] [--out profiles/patch_embed_bench.txt]

Prints one JSON line and writes the table to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--embed", type=int, default=96)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "patch_embed_bench.txt"))
    a = ap.parse_args()
    import time
    import torch
    from mtlora_amd import swin_transformer_mtlora as S
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mod = S.PatchEmbed(img_size=a.size, patch_size=4, in_chans=3, embed_dim=a.embed, norm_layer=torch.nn.LayerNorm).to(dev)
    img = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    M = a.batch * (a.size // 4) ** 2
    gy = torch.randn(a.batch, M // a.batch, a.embed, device=dev)

    def step(on, train):
        S.PATCH_EMBED = on
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if not train:
                with torch.no_grad():
                    return mod(img)
            y = mod(img)
        mod.zero_grad(set_to_none=True)
        y.backward(gy)
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

    prev = S.PATCH_EMBED
    try:
        y1, g1 = step(True, True).float(), [p.grad.clone() for p in mod.parameters()]
        y0, g0 = step(False, True).float(), [p.grad.clone() for p in mod.parameters()]
        diff = {"y": ((y1 - y0).abs().max() / y0.abs().max()).item(),
                "grads": max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(g1, g0))}
        t = {k: [] for k in ("fused", "separate", "fused_fwd", "separate_fwd")}
        issue = {k: [] for k in t}
        for _ in range(a.rounds):  # the routes alternate, so that a drift of the box shows in both
            for k, on, train in (("fused", True, True), ("separate", False, True), ("fused_fwd", True, False), ("separate_fwd", False, False)):
                us, host_us = timed(on, train)
                t[k].append(us)
                issue[k].append(host_us)
    finally:
        S.PATCH_EMBED = prev
    best = {k: min(v) for k, v in t.items()}
    host = {k: min(v) for k, v in issue.items()}
    img_b, tok_b = img.numel() * 4, M * a.embed * 4
    res = {"batch": a.batch, "size": a.size, "embed": a.embed, "M": M, "us": best, "host_issue_us": host, "us_rounds": t, "rel_diff_fused_vs_separate": diff,
           "bytes_fwd": img_b + tok_b, "bytes_fwd_bwd": 2 * (img_b + tok_b), "device": torch.cuda.get_device_name(0)}
    lines = [f"# tools/bench_patch_embed.py --batch {a.batch} --size {a.size} --embed {a.embed} --steps {a.steps} --warmup {a.warmup} "
             f"--inner {a.inner} --rounds {a.rounds}",
             f"# {res['device']}; bf16 autocast, fp32 image and tokens, M = {M}; us per call by device events, and the host time to issue a call, median of {a.steps} "
             f"windows of {a.inner} calls after {a.warmup} warm-up, best of {a.rounds} alternating rounds",
             f"# {'pass':<10s} {'fused us':>10s} {'(issue us)':>11s} {'separate us':>12s} {'(issue us)':>11s} {'speed-up':>9s} {'fused TB/s':>11s}"]
    for name, f, s, b in (("fwd+bwd", "fused", "separate", res["bytes_fwd_bwd"]), ("fwd", "fused_fwd", "separate_fwd", res["bytes_fwd"])):
        lines.append(f"  {name:<10s} {best[f]:10.1f} {host[f]:11.1f} {best[s]:12.1f} {host[s]:11.1f} {best[s] / best[f]:9.2f} "
                     f"{b / (best[f] * 1e-6) / 1e12:11.3f}")
    lines.append(f"# fused against separate on the same inputs, relative to max |separate|: y {diff['y']:.2e}, gradients {diff['grads']:.2e}")
    lines.append(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
