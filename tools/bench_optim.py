"""A/B of the parameter update on a config's trainable set with synthetic gradients: clip_grad_norm_(foreach) + torch AdamW(fused)
-- what train_step runs with build_optimizer(impl="torch") -- against FusedAdamW.clip_and_step (impl="hip", csrc/optim.hip).

    python tools/bench_optim.py [--config c2] [--iters 50] [--rounds 5] [--out profiles/optim_ab.txt]

Per call and implementation: HOST time (perf_counter around the call, no synchronisation inside: what the update adds to the
step's issue time) and DEVICE time (HIP events around the call on the launch stream; where the host issues slower than the GPU
executes this is the issue-bound span, not the kernels' sum).  The two implementations alternate in rounds inside one process;
the medians over all timed calls are reported.  The gradients alternate between two sets of buffers, so the gradient pointers
change from call to call as they do after zero_grad(set_to_none=True).  Needs a GPU: there is no CPU fallback to time.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29  # the copy ceiling the project quotes for the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "optim_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU")
    from mtlora_amd import mtl_harness as H
    dev = torch.device("cuda:0")
    side = {}
    for impl in ("torch", "hip"):
        model = H.build_config_model(a.config, seed=0).to(dev).train()
        opt = H.build_optimizer(model, lr=5e-4, impl=impl)
        ps = [p for g in opt.param_groups for p in g["params"]]
        gen = torch.Generator(device=dev).manual_seed(1)
        grads = [[torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in ps] for _ in range(2)]
        side[impl] = (opt, ps, grads, [], [], [])
    n_tensors, n_elems = len(side["hip"][1]), sum(p.numel() for p in side["hip"][1])

    def call(impl, k, timed):
        opt, ps, grads, host, events, norms = side[impl]
        for p, g in zip(ps, grads[k & 1]):
            p.grad = g
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        if impl == "torch":
            norm = torch.nn.utils.clip_grad_norm_(ps, 5.0, foreach=True)
            opt.step()
        else:
            norm = opt.clip_and_step(5.0)
        e1.record()
        t1 = time.perf_counter()
        if timed:
            host.append((t1 - t0) * 1e3)
            events.append((e0, e1))
        norms.append(norm)

    for impl in side:
        for k in range(a.warmup):
            call(impl, k, False)
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for impl in ("torch", "hip"):
            for k in range(a.iters):
                call(impl, k, True)
            torch.cuda.synchronize()
    res = {}
    for impl, (opt, ps, grads, host, events, norms) in side.items():
        devms = [e0.elapsed_time(e1) for e0, e1 in events]
        res[impl] = (statistics.median(host), min(host), statistics.median(devms), min(devms))
    need = 28.0 * n_elems  # 16 B read (p, g, m, v) + 12 B written (p, m, v) per element
    floor_us = need / (HBM_COPY_TBS * 1e12) * 1e6
    lines = [
        f"bench_optim: clip + AdamW on the trainable set of {a.config}: {n_tensors} tensors, {n_elems} elements",
        f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; one process, the two "
        f"implementations alternating in {a.rounds} rounds of {a.iters} calls after {a.warmup} warm-up calls each",
        "per call                            host ms (median / min)   device ms (median / min)",
    ]
    for impl, what in (("torch", "torch: clip_grad_norm_ + AdamW(fused)"), ("hip", "hip:   FusedAdamW.clip_and_step     ")):
        h, hm, d, dm = res[impl]
        lines.append(f"{what}   {h:8.3f} / {hm:8.3f}        {d:8.3f} / {dm:8.3f}")
    lines.append(f"hip / torch: host {res['hip'][0] / res['torch'][0]:.3f}, device {res['hip'][2] / res['torch'][2]:.3f}")
    lines.append(f"bytes the update must move: 28 B x {n_elems} = {need / 1e6:.2f} MB -> {floor_us:.1f} us at {HBM_COPY_TBS} TB/s; "
                 f"hip device median {res['hip'][2] * 1e3:.1f} us = {need / (res['hip'][2] * 1e-3) / 1e12:.2f} TB/s "
                 f"({100 * floor_us / (res['hip'][2] * 1e3):.0f} % of that ceiling; the span holds three launches, and the norm "
                 "pass reads the gradients once more, 4 B per element, on top of the 28)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
