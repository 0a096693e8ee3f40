"""What a checkpoint costs the replayed train loop: the time the training stream is held up per save, three ways, around ONE captured
step (GraphedTrainStep, fp16 autocast with the LossScaler, FusedAdamW with a cosine schedule inside the graph) at c2:

  (a) none      a window of --iters replays, nothing saved
  (b) blocking  the same window with, after its middle replay, the reference's save (utils.py:280-294; save_checkpoint without
                state=): model.state_dict() + optimizer.state_dict() + loss_scaler.state_dict() + torch.save, all on the loop's thread
  (c) snapshot  the same window with save_checkpoint(state=TrainState, blocking=False): one pack launch on the training stream, one
                asynchronous copy to pinned memory, the file written by the background thread while the loop goes on
                (wait_for_saves() after the window, outside the clock: the file is complete before the next round)

    python tools/bench_checkpoint.py [--config c2] [--iters 20] [--rounds 5] [--warmup 10] [--legs abc] [--out profiles/checkpoint_bench.txt]

Per leg and round: the host clock around the window, ending in a device synchronise.  Reported per leg: the median window and,
for (b) and (c), the stall per save = median window - median window of (a).  Then the two device-side pieces of (c) on their own,
timed with events over --rounds repeats: the pack kernel (bytes gathered / time, next to the copy rate DESIGN 7 quotes) and the
device-to-host copy of the packed buffer.  The pack is timed twice: repeated back to back (its 2 x 104 MB at c2 fit the 256 MiB
Infinity Cache, so this is a warm figure) and after a 512 MiB fill of another buffer in front of every repeat, which is the state a
train step leaves the caches in.  Needs a GPU.
"""
import argparse
import logging
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(a):
    from mtlora_amd import checkpoint as C
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.lr_scheduler import CosineLRScheduler
    from mtlora_amd.optim import LossScaler
    dev = torch.device("cuda:0")
    cfg = H.config(a.config)
    tasks = list(cfg["tasks"])
    torch.manual_seed(0)
    img, tg = H.synthetic_batch(cfg["batch"], cfg["img_size"], tasks, seed=1, device=dev)
    model = H.build_config_model(a.config, seed=0).to(dev).train()
    opt = H.build_optimizer(model, lr=5e-4, impl="hip", capturable=True)
    sched = CosineLRScheduler(opt, t_initial=1000000, lr_min=1e-6, warmup_t=5, warmup_lr_init=1e-7, t_in_epochs=False)
    scaler = LossScaler(init_scale=2.0 ** 10)
    step = H.GraphedTrainStep(model, H.MultiTaskLoss(tasks), opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler,
                              lr_scheduler=sched)
    if not step.graphed:
        raise SystemExit(f"bench_checkpoint: the step was not captured: {step.why}")
    state = C.TrainState(model, opt, sched, scaler)
    return dict(step=step, model=model, opt=opt, sched=sched, scaler=scaler, state=state)


def window(leg, s, a, config, epoch, log):
    from mtlora_amd import checkpoint as C
    step = s["step"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters):
        step()
        if i == a.iters // 2 - 1:
            if leg == "b":
                C.save_checkpoint(config, epoch, s["model"], 0.0, s["opt"], s["sched"], s["scaler"], log)
            elif leg == "c":
                C.save_checkpoint(config, epoch, s["model"], 0.0, s["opt"], s["sched"], s["scaler"], log, state=s["state"], blocking=False)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    C.wait_for_saves()
    return ms


def pieces(s, repeats, cold):
    """the pack launch and the device-to-host copy of one snapshot, each timed alone with events; ms lists and the byte counts.
    ``cold``: 512 MiB are written to another buffer in front of every repeat"""
    from mtlora_amd import _lib as L
    ts = s["state"]
    ts.snapshot().wait()
    lay = ts._layout
    live = sum(n for _, n, _, _ in lay.where.values())
    host = ts._slots[0].host
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=host.device if host.is_cuda else "cuda:0") if cold else None
    torch.cuda.synchronize()
    pack, copy = [], []
    for r in range(repeats):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        if cold:
            flush.fill_(r & 0xFF)
        e0.record()
        L.check(L.lib().mtlora_snapshot_pack(L.ptr(lay.table), lay.n, lay.n_chunks, L.ptr(lay.staging), lay.extent, L.stream_ptr()), "pack")
        e1.record()
        host[:lay.extent].copy_(lay.staging[:lay.extent], non_blocking=True)
        e2.record()
        torch.cuda.synchronize()
        pack.append(e0.elapsed_time(e1))
        copy.append(e1.elapsed_time(e2))
    return pack, copy, live, lay.extent, lay.n, lay.n_chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--out", default=os.path.join("profiles", "checkpoint_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_checkpoint: needs a GPU")
    log = logging.getLogger("bench_checkpoint")
    legs = [l for l in "abc" if l in a.legs]
    s = build(a)
    out_dir = tempfile.mkdtemp(prefix="bench_checkpoint_")
    config = types.SimpleNamespace(OUTPUT=out_dir)
    try:
        for _ in range(a.warmup):
            s["step"]()
        for l in legs:  # one untimed window per leg: pinned buffers, the table and the writer thread come into being here
            window(l, s, a, config, 0, log)
        ms = {l: [] for l in legs}
        for r in range(a.rounds):
            for l in legs:
                ms[l].append(window(l, s, a, config, 1 + r % 2, log))
        sizes = {f: os.path.getsize(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
        pack, copy, live, extent, n, n_chunks = pieces(s, max(a.rounds, 5), cold=False)
        pack_cold = pieces(s, max(a.rounds, 5), cold=True)[0]
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    what = {"a": "(a) none:     replays only                                        ",
            "b": "(b) blocking: state_dict() + torch.save on the loop's thread      ",
            "c": "(c) snapshot: TrainState.snapshot() + background write            "}
    lines = [f"bench_checkpoint: GraphedTrainStep of {a.config}, fp16 + LossScaler + FusedAdamW with the schedule inside the graph",
             f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; one process, the legs alternating "
             f"in {a.rounds} rounds; a window is {a.iters} replays, the save follows replay {a.iters // 2}; files in a temporary directory: "
             + ", ".join(f"{f} {b / 1e6:.1f} MB" for f, b in sizes.items()),
             "ms per window (host clock, device synchronised at the end)            median   spread    rounds"]
    med = {}
    for l in legs:
        med[l] = statistics.median(ms[l])
        lines.append(f"{what[l]}  {med[l]:8.2f} {max(ms[l]) - min(ms[l]):8.2f}    " + " ".join(f"{v:.2f}" for v in ms[l]))
    for l in "bc":
        if l in med and "a" in med:
            lines.append(f"stall per save ({l}) - (a): {med[l] - med['a']:+.2f} ms")
    mp, mc, mpc = statistics.median(pack), statistics.median(copy), statistics.median(pack_cold)
    lines.append(f"snapshot: {n} tensors, {live / 1e6:.2f} MB live in a packed buffer of {extent / 1e6:.2f} MB, {n_chunks} chunks")
    for name, t, m in (("back to back (warm: the bytes fit the Infinity Cache)", pack, mp), ("after a 512 MiB fill of another buffer", pack_cold, mpc)):
        lines.append(f"pack kernel alone, {name}: median {m * 1e3:.1f} us of {len(t)} ({' '.join(f'{v * 1e3:.1f}' for v in t)}): "
                     f"{live / m / 1e6:.1f} GB/s gathered, {2 * live / m / 1e6:.1f} GB/s read + written (DESIGN 7 quotes 6.29 TB/s for a copy)")
    lines.append(f"device-to-host copy alone: median {mc:.3f} ms of {len(copy)} ({' '.join(f'{v:.3f}' for v in copy)}): "
                 f"{extent / mc / 1e6:.1f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
