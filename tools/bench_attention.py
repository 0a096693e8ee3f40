"""Window attention at the window-12 stage shapes of Swin-B / 384 (batch 16, bf16): the library's forward and backward kernels
(csrc/attention_wide.h through functional.WindowAttentionFn, image layout, shifted) against the eager comparator the project uses
everywhere -- the oracle's ATen ops (roll + partition -> core -> merge + roll) under bf16 autocast on the same GPU, run in a process
of its own.

    python tools/bench_attention.py [--batch 16] [--iters 20] [--out profiles/attention_wide_bench.txt]   (--out: relative to the repository)

    python tools/bench_attention.py --attn-drop 0.1 [--batch 16] [--out profiles/attention_dropout_bench.txt]
        the attention-dropout kernels (csrc/attention_dropout.h) next to the plain ones (p = 0) at the C2 stage shapes (Swin-T / 448,
        window 7) and at one window-12 shape, forward and backward, bf16

Device time by HIP events around `iters` back-to-back calls, median of `rounds` such spans.  TB/s is DESIGN section 5's algorithmic
traffic (4 M C es forward, 7 M C es backward) over that time.  Needs a GPU: there is no CPU fallback to time.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = [(96, 4), (48, 8), (24, 16), (12, 32)]  # (H = W, heads) of Swin-B patch4_window12_384
WS = 12


def _span(fn, iters, rounds, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(out)  # us per call


def _inputs(B, HW, nH, dev):
    from mtlora_amd.swin_transformer_mtlora import _shift_mask, _shift_regions
    C, N = nH * 32, WS * WS
    shift = 0 if HW <= WS else WS // 2
    g = torch.Generator(device=dev).manual_seed(HW)
    qkv = (torch.randn(B, HW, HW, 3 * C, device=dev, generator=g) * 0.7).to(torch.bfloat16)
    bias = torch.randn(nH, N, N, device=dev, generator=g) * 0.5
    ids = _shift_regions(HW, HW, WS, shift).to(torch.int32).to(dev) if shift else None
    mask = _shift_mask(HW, HW, WS, shift).to(dev) if shift else None
    gout = (torch.randn(B, HW, HW, C, device=dev, generator=g)).to(torch.bfloat16)
    return qkv, bias, ids, mask, gout, shift


def run(which, B, iters, rounds):
    from mtlora_amd import functional as Fn
    from oracle import mtlora_oracle as O
    dev = torch.device("cuda:0")
    rows = []
    for HW, nH in STAGES:
        qkv, bias, ids, mask, gout, shift = _inputs(B, HW, nH, dev)
        C, N = nH * 32, WS * WS
        scale = 32 ** -0.5
        q = qkv.clone().requires_grad_(True)
        b = bias.clone().requires_grad_(True)
        if which == "hip":
            meta = Fn.AttnMeta(B=B, H=HW, W=HW, window_size=WS, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=scale)

            def fwd():
                return Fn.WindowAttentionFn.apply(meta, q, b, None, ids)
        else:
            def fwd():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    win = O.roll_and_window_partition(q, shift, WS).reshape(-1, N, 3 * C)
                    core = O.window_attention_core(win, b, mask, nH, scale)
                    return O.window_merge_and_roll(core.reshape(-1, WS, WS, C), shift, WS, HW, HW)

        def fwd_nograd():
            with torch.no_grad():
                fwd()

        def both():
            q.grad = b.grad = None
            fwd().backward(gout)

        t_f = _span(fwd_nograd, iters, rounds)
        t_fb = _span(both, iters, rounds)
        rows.append({"HW": HW, "heads": nH, "fwd_us": t_f, "fwd_bwd_us": t_fb})
    return rows


DROP_SHAPES = [(7, 112, 3), (7, 56, 6), (7, 28, 12), (7, 14, 24), (12, 24, 16)]  # (window, H = W, heads): C2 stages 0-3, Swin-B/384 stage 2


def run_drop(p, B, iters, rounds):
    """p = 0 (plain kernels) and p (dropout kernels) at DROP_SHAPES: us per forward / backward call"""
    from mtlora_amd import functional as Fn
    from mtlora_amd.swin_transformer_mtlora import _shift_regions
    dev = torch.device("cuda:0")
    rows = []
    for ws, HW, nH in DROP_SHAPES:
        C, N, shift = nH * 32, ws * ws, (0 if HW <= ws else ws // 2)
        g = torch.Generator(device=dev).manual_seed(HW)
        q = (torch.randn(B, HW, HW, 3 * C, device=dev, generator=g) * 0.7).to(torch.bfloat16).requires_grad_(True)
        b = (torch.randn(nH, N, N, device=dev, generator=g) * 0.5).requires_grad_(True)
        ids = _shift_regions(HW, HW, ws, shift).to(torch.int32).to(dev) if shift else None
        gout = torch.randn(B, HW, HW, C, device=dev, generator=g).to(torch.bfloat16)
        meta = Fn.AttnMeta(B=B, H=HW, W=HW, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=32 ** -0.5)
        row = {"ws": ws, "HW": HW, "heads": nH}
        for tag, pp in (("p0", 0.0), ("drop", p)):
            def fwd():
                return Fn.WindowAttentionFn.apply(meta, q, b, None, ids, pp, 1234)

            def fwd_nograd():
                with torch.no_grad():
                    fwd()

            def both():
                q.grad = b.grad = None
                fwd().backward(gout)

            row[tag + "_fwd_us"] = _span(fwd_nograd, iters, rounds)
            row[tag + "_fwd_bwd_us"] = _span(both, iters, rounds)
        rows.append(row)
    return rows


def main_drop(a):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "drop", "--attn-drop", str(a.attn_drop), "--batch",
                            str(a.batch), "--iters", str(a.iters), "--rounds", str(a.rounds)], capture_output=True, text=True, cwd=ROOT,
                           timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_attention: the child did not finish within {a.child_timeout} s")
    line = [l for l in p.stdout.splitlines() if l.startswith("ROWS ")]
    if p.returncode != 0 or not line:
        raise SystemExit(f"bench_attention: the child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    lines = [
        f"bench_attention --attn-drop {a.attn_drop}: attention dropout kernels against the plain kernels (p = 0), batch {a.batch}, bf16, image "
        "layout, shifted + region ids",
        f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; device time by HIP events, "
        f"median of {a.rounds} spans of {a.iters} calls; backward = (forward + backward) - forward",
        " ws  HxW     heads |  p=0 fwd us  drop fwd us  ratio |  p=0 bwd us  drop bwd us  ratio",
    ]
    for r in json.loads(line[0][5:]):
        b0, b1 = r["p0_fwd_bwd_us"] - r["p0_fwd_us"], r["drop_fwd_bwd_us"] - r["drop_fwd_us"]
        lines.append(f"{r['ws']:3d}  {r['HW']:3d}x{r['HW']:<3d} {r['heads']:5d} | {r['p0_fwd_us']:11.1f} {r['drop_fwd_us']:12.1f} "
                     f"{r['drop_fwd_us'] / r['p0_fwd_us']:6.2f} | {b0:11.1f} {b1:12.1f} {b1 / b0:6.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "attention_wide_bench.txt"))
    ap.add_argument("--child-timeout", type=float, default=150.0, help="seconds each of the two measuring processes may take")
    ap.add_argument("--child", choices=["hip", "eager", "drop"])
    ap.add_argument("--attn-drop", type=float, default=0.0, help="time the attention-dropout kernels with this p next to the plain ones")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention: needs a GPU")
    if a.child == "drop":
        print("ROWS " + json.dumps(run_drop(a.attn_drop, a.batch, a.iters, a.rounds)))
        return
    if a.attn_drop > 0.0:
        return main_drop(a)
    if a.child:
        print("ROWS " + json.dumps(run(a.child, a.batch, a.iters, a.rounds)))
        return
    res = {}
    for which in ("hip", "eager"):  # one process each, one after the other
        try:  # a child that does not finish is killed: nothing else is started on the GPU after it
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--batch", str(a.batch), "--iters", str(a.iters),
                                "--rounds", str(a.rounds)], capture_output=True, text=True, cwd=ROOT, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_attention: {which} child did not finish within {a.child_timeout} s")
        line = [l for l in p.stdout.splitlines() if l.startswith("ROWS ")]
        if p.returncode != 0 or not line:
            raise SystemExit(f"bench_attention: {which} child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        res[which] = json.loads(line[0][5:])
    lines = [
        f"bench_attention: window {WS} x {WS} attention, Swin-B/384 stage shapes, batch {a.batch}, bf16, shifted (stage 3: one window, no shift)",
        f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; device time by HIP events, "
        f"median of {a.rounds} spans of {a.iters} calls; backward = (forward + backward) - forward",
        "stage  HxW    heads      M      C |  hip fwd us  TB/s(4MC) |  hip bwd us  TB/s(7MC) | eager fwd us  eager bwd us | eager/hip fwd  bwd",
    ]
    for k, (HW, nH) in enumerate(STAGES):
        M, C = a.batch * HW * HW, nH * 32
        h, e = res["hip"][k], res["eager"][k]
        hb, eb = h["fwd_bwd_us"] - h["fwd_us"], e["fwd_bwd_us"] - e["fwd_us"]
        lines.append(f"{k:5d}  {HW:3d}x{HW:<3d} {nH:5d} {M:6d} {C:6d} | {h['fwd_us']:10.1f} {4 * M * C * 2 / h['fwd_us'] / 1e6:10.3f} | "
                     f"{hb:10.1f} {7 * M * C * 2 / hb / 1e6:10.3f} | {e['fwd_us']:12.1f} {eb:12.1f} | {e['fwd_us'] / h['fwd_us']:13.2f} {eb / hb:4.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out)  # (relative to the repository, like the children's cwd)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
