#!/usr/bin/env python
"""Decoder front end, isolated: the stages' tokens to the head's (B H W, ld) pixel matrix, one task.

  fused     mtl_harness.DECODER_FRONT on: functional.DecoderFrontFn, one launch forward, three backward (csrc/decoder_front.hip)
  separate  the separate steps: four linear_big_m (rank-0 mtlora_linear_fwd / _bwd, weight casts, weight gradients) and
            ConcatUpsampleFn (slice copy, pad fills, three upsample launches each way)

Both routes run in one process on the same tokens and weights, alternating, bf16 autocast, at the stage geometry of Swin-T (c2:
B = 32, 448 px: grids 56 / 28 / 14 / 14, C = 192 / 384 / 768 / 768, c = 18 / 36 / 72 / 144).  Timed with device events around --inner
back-to-back calls; reported: the median over --steps windows and their spread (max - min), the best of --rounds alternating
rounds.  `fwd+bwd` forms the gradients of the tokens and of the four weights; `fwd` runs under torch.no_grad().  The launch counts
come from the library's own per-launch records (mtlora_prof_begin / _end) and cover its kernels only, not ATen's.

    python tools/bench_decoder_front.py [--batch 32] [--res 56] [--steps 10] [--warmup 3] [--inner 20] [--rounds 3] [--band 0]
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
    ap.add_argument("--res", type=int, default=56, help="finest token grid (56 at 448 px)")
    ap.add_argument("--embed", type=int, default=96)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "decoder_front_bench.txt"))
    a = ap.parse_args()
    import ctypes
    import torch
    from mtlora_amd import _lib as L
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dims = [a.embed * 2, a.embed * 4, a.embed * 8, a.embed * 8]
    res = [a.res, a.res // 2, a.res // 4, a.res // 4]
    chans = (18, 36, 72, 144)
    down = H.Downsampler(dims, chans, res).to(dev)
    feats = [torch.randn(a.batch, r * r, d, device=dev).bfloat16().requires_grad_(True) for r, d in zip(res, dims)]
    _, ld = Fn.ConcatUpsampleFn.layout(chans)
    gy = torch.randn(a.batch * a.res * a.res, ld, device=dev).bfloat16()

    def matrix(on):
        H.DECODER_FRONT = on
        out = down(feats)
        if isinstance(out, H.DecoderFront):
            return out.t
        assert not on, "the fused path refused the benchmark's shape"
        return Fn.ConcatUpsampleFn.apply(*[m.permute(0, 2, 3, 1) for m in out])

    def step(on, train):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if not train:
                with torch.no_grad():
                    return matrix(on)
            y = matrix(on)
        for t in feats + list(down.parameters()):
            t.grad = None
        y.backward(gy)
        return y

    def timed(on, train):
        for _ in range(a.warmup):
            step(on, train)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                step(on, train)
            e1.record()
            torch.cuda.synchronize()
            ms.append(1e3 * e0.elapsed_time(e1) / a.inner)
        return statistics.median(ms), max(ms) - min(ms)

    def launches(on, train):
        L.lib().mtlora_prof_begin(4096)
        step(on, train)
        torch.cuda.synchronize()
        s = L.ProfSummary()
        L.lib().mtlora_prof_end(ctypes.byref(s))
        return int(sum(s.count))

    prev = H.DECODER_FRONT
    legs = (("fused", True, True), ("separate", False, True), ("fused_fwd", True, False), ("separate_fwd", False, False))
    try:
        y1, g1 = step(True, True).float(), [t.grad.float().clone() for t in feats + list(down.parameters())]
        y0, g0 = step(False, True).float(), [t.grad.float().clone() for t in feats + list(down.parameters())]
        diff = {"y": ((y1 - y0).abs().max() / y0.abs().max()).item(),
                "grads": max(((u - v).abs().max() / v.abs().max()).item() for u, v in zip(g1, g0))}
        counts = {k: launches(on, train) for k, on, train in legs}
        t = {k: [] for k, _, _ in legs}
        for _ in range(a.rounds):  # the routes alternate, so that a drift of the box shows in both
            for k, on, train in legs:
                t[k].append(timed(on, train))
    finally:
        H.DECODER_FRONT = prev
    best = {k: min(v) for k, v in t.items()}  # (median us, spread us) of the best round
    out = {"batch": a.batch, "res": a.res, "dims": dims, "chans": chans, "us_median_spread": best, "us_rounds": t, "library_launches": counts,
           "rel_diff_fused_vs_separate": diff, "device": torch.cuda.get_device_name(0)}
    lines = [f"# tools/bench_decoder_front.py --batch {a.batch} --res {a.res} --embed {a.embed} --steps {a.steps} --warmup {a.warmup} "
             f"--inner {a.inner} --rounds {a.rounds}",
             f"# {out['device']}; bf16 autocast; us per call by device events: median (spread) of {a.steps} windows of {a.inner} calls after "
             f"{a.warmup} warm-up, best of {a.rounds} alternating rounds; launches: the library's kernels per call",
             f"# {'pass':<10s} {'fused us':>18s} {'launches':>9s} {'separate us':>18s} {'launches':>9s} {'speed-up':>9s}"]
    for name, f, s in (("fwd+bwd", "fused", "separate"), ("fwd", "fused_fwd", "separate_fwd")):
        lines.append(f"  {name:<10s} {best[f][0]:10.1f} ({best[f][1]:5.1f}) {counts[f]:9d} {best[s][0]:10.1f} ({best[s][1]:5.1f}) {counts[s]:9d} "
                     f"{best[s][0] / best[f][0]:9.2f}")
    lines.append(f"# fused against separate on the same inputs, relative to max |separate|: y {diff['y']:.2e}, gradients {diff['grads']:.2e}")
    lines.append(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
