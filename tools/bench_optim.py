"""A/B of the parameter update on a config's trainable set with synthetic gradients: clip_grad_norm_(foreach) + torch AdamW(fused)
-- what train_step runs with build_optimizer(impl="torch") -- against FusedAdamW.clip_and_step (impl="hip", csrc/optim.hip).

    python tools/bench_optim.py [--config c2] [--iters 50] [--rounds 5] [--out profiles/optim_ab.txt]
    python tools/bench_optim.py --graph [--config c2] [--iters 200] [--runs 3] [--out profiles/optim_graph_ab.txt]

Per call and implementation: HOST time (perf_counter around the call, no synchronisation inside: what the update adds to the
step's issue time) and DEVICE time (HIP events around the call on the launch stream; where the host issues slower than the GPU
executes this is the issue-bound span, not the kernels' sum).  The two implementations alternate in rounds inside one process;
the medians over all timed calls are reported.  The gradients alternate between two sets of buffers, so the gradient pointers
change from call to call as they do after zero_grad(set_to_none=True).  Needs a GPU: there is no CPU fallback to time.

``--graph``: the update as it runs inside ``GraphedTrainStep`` -- captured once in a HIP graph and REPLAYED: clip_grad_norm_(foreach)
+ torch AdamW(fused, capturable=True), what the graph held before, against FusedAdamW(capturable=True).clip_and_step, whose
learning rate is set anew and pushed to the device before every replay (the torch graph cannot follow it).  Gradients in static
buffers.  Each leg runs in a process of its own, ``--runs`` times, alternating; per leg the median over its replays of the DEVICE
time (HIP events around the replay) and of the HOST time of one replay (with push_hyperparameters() and bump_versions() for the
fused leg), then the median and the spread (max - min) over the runs.

``--graph --schedule``: what the device-side LR schedule takes off the host.  Two FusedAdamW legs under the same cosine schedule
(mtlora_amd.lr_scheduler): ``hip`` steps the host scheduler and pushes the new lr in front of every replay, ``hipsched`` has the
schedule attached (FusedAdamW.attach_schedule) and only replays.  Same columns; written to profiles/optim_graph_schedule.txt.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29  # the copy ceiling the project quotes for the MI355X
# --optim: (the fused class, what the torch leg runs -- torch has no LAMB: its AdamW is the yardstick there --, bytes per element
# the update must move, and how they add up)
OPTIMS = {"adamw": ("FusedAdamW", "adamw", "AdamW", 28, "16 B read (p, g, m, v) + 12 B written (p, m, v)"),
          "sgd": ("FusedSGD", "sgd", "SGD(nesterov, foreach)", 20, "12 B read (p, g, buf) + 8 B written (p, buf)"),
          "lamb": ("FusedLAMB", "adamw", "AdamW", 40, "moments: 16 B read (p, g, m, v) + 8 B written (m, v); apply: 12 B read (p, m, v) "
                   "again + 4 B written (p)")}


def build(H, model, impl, a, capturable=False):
    return H.build_optimizer(model, lr=5e-4, impl=impl, capturable=capturable, name=a.optim if impl == "hip" else OPTIMS[a.optim][1])


def graph_leg(a):
    """one leg of --graph in this process: capture the update once, replay it; prints one GRAPH_LEG json line"""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.lr_scheduler import CosineLRScheduler
    leg, dev = a.graph_leg, torch.device("cuda:0")
    impl = "hip" if leg == "hipsched" else leg
    model = H.build_config_model(a.config, seed=0).to(dev).train()
    opt = build(H, model, impl, a, capturable=True)
    sched = None
    if a.schedule and impl == "hip":  # (long enough that the timed replays stay on the cosine segment)
        sched = CosineLRScheduler(opt, t_initial=100 * (a.iters + a.warmup), lr_min=1e-6, warmup_t=5, warmup_lr_init=1e-7, t_in_epochs=False)
        if leg == "hipsched":
            opt.attach_schedule(sched)
    ps = [p for g in opt.param_groups for p in g["params"]]
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2  # static buffers: the graph holds their addresses

    def update():
        if impl == "torch":
            torch.nn.utils.clip_grad_norm_(ps, 5.0, foreach=True)
            opt.step()
        else:
            opt.clip_and_step(5.0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()

    def replay(k):
        if leg == "hipsched":  # the schedule is in the graph: nothing to do on the host
            pass
        elif sched is not None:  # the host scheduler steps, the new lr is pushed
            sched.step_update(k)
            opt.push_hyperparameters()
        elif impl == "hip":  # a moving learning rate: set, pushed (one small copy in front of the replay), replayed
            for g in opt.param_groups:
                g["lr"] = 5e-4 * (1.0 - 1e-4 * k)
            opt.push_hyperparameters()
        graph.replay()
        if impl == "hip":
            opt.bump_versions()

    for k in range(a.warmup):
        replay(k)
    torch.cuda.synchronize()
    host, events = [], []
    w0 = time.perf_counter()
    for k in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        replay(a.warmup + k)
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        events.append((e0, e1))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - w0) * 1e3 / a.iters
    devms = [e0.elapsed_time(e1) for e0, e1 in events]
    finite = all(bool(torch.isfinite(p).all()) for p in ps)
    print("GRAPH_LEG " + json.dumps({"impl": leg, "device_ms": statistics.median(devms), "host_ms": statistics.median(host),
                                     "wall_ms": wall, "finite": finite, "tensors": len(ps), "elements": sum(p.numel() for p in ps),
                                     "gpu": torch.cuda.get_device_name(0)}), flush=True)


def graph_ab(a):
    """--graph: the two legs alternate, each in a fresh child process (this process never opens the GPU)"""
    if a.schedule:
        return schedule_ab(a)
    rows = {"torch": [], "hip": []}
    for _ in range(a.runs):
        for impl in ("torch", "hip"):
            cmd = [sys.executable, os.path.abspath(__file__), "--graph-leg", impl, "--config", a.config, "--iters", str(a.iters),
                   "--warmup", str(a.warmup), "--optim", a.optim]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("GRAPH_LEG ")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench_optim: the {impl} leg failed (exit {r.returncode}):\n{r.stderr[-2000:]}")
            rows[impl].append(json.loads(line[-1][len("GRAPH_LEG "):]))
            print(f"  run {len(rows[impl])} {impl}: device {rows[impl][-1]['device_ms']:.4f} ms per replay", flush=True)
            if not rows[impl][-1]["finite"]:
                raise SystemExit(f"bench_optim: the {impl} leg left non-finite parameters")
    one = rows["hip"][0]
    fused, _, torch_what, _, _ = OPTIMS[a.optim]
    lines = [f"bench_optim --graph: clip + {fused[5:]} REPLAYED from a HIP graph on the trainable set of {a.config}: {one['tensors']} tensors, "
             f"{one['elements']} elements",
             f"box: {one['gpu']}, torch {torch.__version__}, HIP {torch.version.hip}; each leg in its own process, {a.runs} runs each, "
             f"alternating; {a.iters} timed replays after {a.warmup} warm-up replays",
             "per replay                                        device ms            host ms              wall ms (iters / sync)",
             "                                                  median  spread       median  spread       median  spread"]
    med = {}
    for impl, what in (("torch", f"torch: clip_grad_norm_ + {torch_what}".ljust(46)), ("hip", f"hip:   {fused}(capturable).clip_and_step".ljust(46))):
        cols = []
        for key in ("device_ms", "host_ms", "wall_ms"):
            v = [r[key] for r in rows[impl]]
            med[impl, key] = statistics.median(v)
            cols.append(f"{med[impl, key]:8.4f} {max(v) - min(v):7.4f}")
        lines.append(f"{what}   " + "     ".join(cols) + "    runs (device): " + " ".join(f"{r['device_ms']:.4f}" for r in rows[impl]))
    lines.append(f"hip / torch: device {med['hip', 'device_ms'] / med['torch', 'device_ms']:.3f}, host "
                 f"{med['hip', 'host_ms'] / med['torch', 'host_ms']:.3f}, wall {med['hip', 'wall_ms'] / med['torch', 'wall_ms']:.3f} "
                 "(the fused leg's host time includes setting and pushing a new learning rate before every replay)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def schedule_ab(a):
    """--graph --schedule: per-step push against the schedule inside the graph; each leg in a fresh child process, alternating"""
    rows = {"hip": [], "hipsched": []}
    for _ in range(a.runs):
        for leg in rows:
            cmd = [sys.executable, os.path.abspath(__file__), "--graph-leg", leg, "--schedule", "--config", a.config, "--iters",
                   str(a.iters), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("GRAPH_LEG ")]
            if r.returncode != 0 or not line:
                raise SystemExit(f"bench_optim: the {leg} leg failed (exit {r.returncode}):\n{r.stderr[-2000:]}")
            rows[leg].append(json.loads(line[-1][len("GRAPH_LEG "):]))
            if not rows[leg][-1]["finite"]:
                raise SystemExit(f"bench_optim: the {leg} leg left non-finite parameters")
    one = rows["hip"][0]
    lines = [f"bench_optim --graph --schedule: FusedAdamW.clip_and_step REPLAYED under a cosine schedule on the trainable set of "
             f"{a.config}: {one['tensors']} tensors, {one['elements']} elements",
             f"box: {one['gpu']}, torch {torch.__version__}, HIP {torch.version.hip}; each leg in its own process, {a.runs} runs each, "
             f"alternating; {a.iters} timed replays after {a.warmup} warm-up replays",
             "per replay                                               device ms            host ms              wall ms (iters / sync)",
             "                                                         median  spread       median  spread       median  spread"]
    med = {}
    for leg, what in (("hip", "host: step_update + push_hyperparameters + replay     "),
                      ("hipsched", "device: attach_schedule, replay only                  ")):
        cols = []
        for key in ("device_ms", "host_ms", "wall_ms"):
            v = [r[key] for r in rows[leg]]
            med[leg, key] = statistics.median(v)
            cols.append(f"{med[leg, key]:8.4f} {max(v) - min(v):7.4f}")
        lines.append(f"{what}   " + "     ".join(cols))
    lines.append(f"host time saved per replay: {(med['hip', 'host_ms'] - med['hipsched', 'host_ms']) * 1e3:.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--iters", type=int, default=0, help="timed calls per round (default 50), or timed replays per --graph leg (200)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graph", action="store_true", help="A/B of the update replayed from a HIP graph, each leg in its own process")
    ap.add_argument("--runs", type=int, default=3, help="--graph: runs per leg")
    ap.add_argument("--schedule", action="store_true", help="--graph: host scheduler + per-step push against the device-side schedule")
    ap.add_argument("--graph-leg", choices=("torch", "hip", "hipsched"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--optim", choices=tuple(OPTIMS), default="adamw", help="which fused optimizer (build_optimizer(name=))")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.schedule and a.optim != "adamw":
        raise SystemExit("bench_optim: --schedule is FusedAdamW's (the other classes have no device-side schedule)")
    a.iters = a.iters or (200 if (a.graph or a.graph_leg) else 50)
    name = ("optim_graph_schedule" if a.schedule else "optim_graph_ab") if a.graph else "optim_ab"
    a.out = a.out or os.path.join("profiles", name + ("" if a.optim == "adamw" else "_" + a.optim) + ".txt")
    if a.graph:
        return graph_ab(a)
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU")
    if a.graph_leg:
        return graph_leg(a)
    from mtlora_amd import mtl_harness as H
    dev = torch.device("cuda:0")
    side = {}
    for impl in ("torch", "hip"):
        model = H.build_config_model(a.config, seed=0).to(dev).train()
        opt = build(H, model, impl, a)
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
    fused, _, torch_what, per_elem, how = OPTIMS[a.optim]
    need = float(per_elem) * n_elems  # per element: see OPTIMS
    launches = "four" if a.optim == "lamb" else "three"
    floor_us = need / (HBM_COPY_TBS * 1e12) * 1e6
    lines = [
        f"bench_optim: clip + {fused[5:]} on the trainable set of {a.config}: {n_tensors} tensors, {n_elems} elements",
        f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; one process, the two "
        f"implementations alternating in {a.rounds} rounds of {a.iters} calls after {a.warmup} warm-up calls each",
        "per call                            host ms (median / min)   device ms (median / min)",
    ]
    for impl, what in (("torch", f"torch: clip_grad_norm_ + {torch_what + ('(fused)' if OPTIMS[a.optim][1] == 'adamw' else '')}"),
                       ("hip", f"hip:   {fused}.clip_and_step".ljust(37))):
        h, hm, d, dm = res[impl]
        lines.append(f"{what}   {h:8.3f} / {hm:8.3f}        {d:8.3f} / {dm:8.3f}")
    lines.append(f"hip / torch: host {res['hip'][0] / res['torch'][0]:.3f}, device {res['hip'][2] / res['torch'][2]:.3f}")
    lines.append(f"bytes the update must move: {per_elem} B ({how}) x {n_elems} = {need / 1e6:.2f} MB -> {floor_us:.1f} us at {HBM_COPY_TBS} TB/s; "
                 f"hip device median {res['hip'][2] * 1e3:.1f} us = {need / (res['hip'][2] * 1e-3) / 1e12:.2f} TB/s "
                 f"({100 * floor_us / (res['hip'][2] * 1e3):.0f} % of that ceiling; the span holds {launches} launches, and the norm "
                 f"pass reads the gradients once more, 4 B per element, on top of the {per_elem})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
