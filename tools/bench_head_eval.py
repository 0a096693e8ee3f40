#!/usr/bin/env python
"""Time the eval-mode decoder head of the c2 model (B = 32: M = 401 408 pixels, 272 padded input channels, 1080 hidden, bf16) on
the same tensors, both ways, alternating in one process per head:

  fused      Fn.head_eval: conv -> BatchNorm (running statistics) -> ReLU -> conv in one launch (csrc/head_eval.hip)
  four-step  what HighResolutionHead.forward runs otherwise under no_grad: F.linear, F.batch_norm, F.relu, F.linear on the
             (M, 1080) hidden matrix (the first weight already scattered to the padded layout, the second padded to 8 classes)

for the four PASCAL heads (21, 3, 1, 7 classes).  HIP events after warm-up, median of --steps, best of --rounds alternating rounds;
the rate is M * (ldx + ncp) * 2 bytes -- what the fused call must move -- over the time.  Each head is measured by a child process
under its own time limit; the first child that fails ends the run.

    python tools/bench_head_eval.py [--batch 32] [--steps 10] [--warmup 3] [--rounds 2] [--out profiles/head_eval_ab.txt]

Prints one JSON line and writes the table to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADS = (("semseg", 21), ("normals", 3), ("sal", 1), ("human_parts", 7))
LDX, HD, PIXELS = 272, 1080, 112 * 112


def measure(a, classes):
    import torch
    import torch.nn.functional as F
    from mtlora_amd import functional as Fn
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    torch.manual_seed(classes)
    M, ncp = a.batch * PIXELS, classes + (-classes) % 8
    x = torch.randn(M, LDX, device=dev).to(dt)
    w1p, b1 = (torch.randn(HD, LDX, device=dev) / LDX ** 0.5).to(dt), 0.1 * torch.randn(HD, device=dev)
    mean, var = 0.3 * torch.randn(HD, device=dev), 0.5 + torch.rand(HD, device=dev)
    gamma, beta = 1 + 0.2 * torch.randn(HD, device=dev), 0.3 * torch.randn(HD, device=dev)
    w2p, b2 = torch.zeros(ncp, HD, device=dev, dtype=dt), torch.zeros(ncp, device=dev)
    w2p[:classes], b2[:classes] = (torch.randn(classes, HD, device=dev) / HD ** 0.5).to(dt), 0.1 * torch.randn(classes, device=dev)
    av = gamma / torch.sqrt(var + 1e-5)
    cv = beta + (b1 - mean) * av
    b1h, b2h = b1.to(dt), b2.to(dt)

    def fused():
        return Fn.head_eval(x, w1p, av, cv, w2p, b2)

    def four():
        h = F.relu(F.batch_norm(F.linear(x, w1p, b1h), mean, var, gamma, beta, False, 0.1, 1e-5))
        return F.linear(h, w2p, b2h)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    with torch.no_grad():
        diff = ((fused().float() - four().float()).abs().max() / four().float().abs().max()).item()
        f, o = [], []
        for _ in range(a.rounds):  # the two routes alternate, so that a drift of the box shows in both
            f.append(timed(fused))
            o.append(timed(four))
    return {"classes": classes, "ncp": ncp, "M": M, "fused_us": 1e3 * min(f), "four_step_us": 1e3 * min(o), "fused_us_rounds": [1e3 * v for v in f],
            "four_step_us_rounds": [1e3 * v for v in o], "bytes": M * (LDX + ncp) * 2, "rel_diff": diff, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per head")
    ap.add_argument("--out", default=os.path.join("profiles", "head_eval_ab.txt"))
    ap.add_argument("--one", type=int, default=0, help="(child) measure the head with this many classes, print its JSON")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a, a.one)))
        return
    rows = []
    for task, classes in HEADS:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(classes), "--batch", str(a.batch), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit(f"bench_head_eval: the {task} head failed (exit {r.returncode}); nothing more is started\n{r.stdout}\n{r.stderr}")
        rows.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), task=task))
    lines = [f"# tools/bench_head_eval.py --batch {a.batch} --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}",
             f"# {rows[0]['device']}; bf16, M = {rows[0]['M']}, {LDX} -> {HD} -> classes; us per call, median of {a.steps} after {a.warmup} "
             f"warm-up, best of {a.rounds} alternating rounds; rate = M (ldx + ncp) 2 bytes / fused time",
             f"# {'head':<12s} {'classes':>7s} {'fused us':>10s} {'four-step us':>13s} {'speed-up':>9s} {'TB/s':>7s} {'max rel diff':>13s}"]
    for r in rows:
        lines.append(f"  {r['task']:<12s} {r['classes']:7d} {r['fused_us']:10.1f} {r['four_step_us']:13.1f} {r['four_step_us'] / r['fused_us']:9.2f} "
                     f"{r['bytes'] / (r['fused_us'] * 1e-6) / 1e12:7.3f} {r['rel_diff']:13.2e}")
    lines.append(json.dumps({"batch": a.batch, "steps": a.steps, "heads": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
