"""What logging costs the replayed train step: three loops over the SAME captured step (GraphedTrainStep, fp16 autocast with the
LossScaler, FusedAdamW with a cosine schedule inside the graph) on the host-bound case, c1 (Swin-T / 224, 1 task, batch 2):

  (a) none     the loop hands over nothing and reads nothing
  (b) items    the reference's loop, main.py:354-401, per step: loss_scaler.state_dict()["scale"], loss.item(), grad_norm.item(),
               every task's loss.item() and the learning rate -- 2 + T host synchronisations in front of the next replay
  (c) meters   GraphedTrainStep(meters=TrainMeters.for_train_step(...)): the meters' update is the graph's last node;
               meters.snapshot() + meters.latest() every --print-freq steps, latest(wait=True) once at the end of the window

    python tools/bench_meters.py [--config c1] [--iters 200] [--rounds 5] [--warmup 20] [--print-freq 10] [--legs abc]
                                 [--out profiles/meters.txt]

(a) and (b) run one captured step WITHOUT meter nodes, (c) a second one with them (its own model and optimizer, same seed); the
legs alternate in rounds inside one process.  Per leg and round: the host clock around --iters calls ending in a device
synchronise, divided by --iters; reported are the median over the rounds and the spread (max - min).  (c) against (a) is what the
meters add to a replay: two small launches (the gather of the step's values, the update).  ``--legs a`` needs nothing of the meters
and so also runs on a tree that does not have them (the same (a) on the commit before).  Needs a GPU.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_step(a, with_meters):
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.lr_scheduler import CosineLRScheduler
    from mtlora_amd.optim import LossScaler
    dev = torch.device("cuda:0")
    cfg = H.config(a.config)
    tasks = list(cfg["tasks"])

    class Keeping(H.MultiTaskLoss):  # the per-task losses of the captured forward: static tensors a replay rewrites
        def combine(self, per):
            self.last_per = per
            return super().combine(per)

    torch.manual_seed(0)
    img, tg = H.synthetic_batch(cfg["batch"], cfg["img_size"], tasks, seed=1, device=dev)
    model = H.build_config_model(a.config, seed=0).to(dev).train()
    opt = H.build_optimizer(model, lr=5e-4, impl="hip", capturable=True)
    total = a.warmup + a.rounds * a.iters * 3 + 16
    sched = CosineLRScheduler(opt, t_initial=100 * total, lr_min=1e-6, warmup_t=5, warmup_lr_init=1e-7, t_in_epochs=False)
    opt.attach_schedule(sched)
    scaler, crit, kw, meters = LossScaler(init_scale=2.0 ** 10), Keeping(tasks), {}, None
    if with_meters:
        from mtlora_amd.meters import TrainMeters
        meters = TrainMeters.for_train_step(tasks, opt, scaler)
        kw = dict(meters=meters)
    step = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, amp_dtype=torch.float16, loss_scaler=scaler,
                              lr_scheduler=sched, **kw)
    if not step.graphed:
        raise SystemExit(f"bench_meters: the step was not captured: {step.why}")
    return dict(step=step, crit=crit, opt=opt, scaler=scaler, meters=meters, tasks=tasks, printed=[])


def run(leg, s, a):
    """--iters calls of one leg, ending in a device synchronise; returns ms per step"""
    step, n_print = s["step"], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters):
        loss = step()
        if leg == "b":  # what main.py:354-401 reads back every step
            row = [s["scaler"].state_dict()["scale"], loss.item(), step.grad_norm.item()]
            row += [s["crit"].last_per[t].item() for t in s["tasks"]]
            row.append(s["opt"].param_groups[0]["lr"])
            if i % a.print_freq == 0:
                n_print += 1
        elif leg == "c" and i % a.print_freq == 0:
            s["meters"].snapshot()
            row = s["meters"].latest()
            n_print += 1
    if leg == "c":
        s["meters"].snapshot()
        row = s["meters"].latest(wait=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.iters
    if leg != "a":
        s["printed"].append((n_print, row))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--out", default=os.path.join("profiles", "meters.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meters: needs a GPU")
    legs = [l for l in "abc" if l in a.legs]
    plain = build_step(a, False) if ("a" in legs or "b" in legs) else None
    metered = build_step(a, True) if "c" in legs else None
    of = {"a": plain, "b": plain, "c": metered}
    for s in {id(v): v for v in of.values() if v is not None}.values():
        for _ in range(a.warmup):
            s["step"]()
    torch.cuda.synchronize()
    ms = {l: [] for l in legs}
    for _ in range(a.rounds):
        for l in legs:
            ms[l].append(run(l, of[l], a))
    what = {"a": "(a) none:   replay only                                   ",
            "b": "(b) items:  the reference's per-step .item() / state_dict ",
            "c": f"(c) meters: in-graph update, snapshot every {a.print_freq:<3d} steps    "}
    lines = [f"bench_meters: GraphedTrainStep of {a.config}, fp16 + LossScaler + FusedAdamW with the schedule inside the graph",
             f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; one process, the legs "
             f"alternating in {a.rounds} rounds of {a.iters} calls after {a.warmup} warm-up calls per step object",
             "ms per step (host clock / calls, device synchronised at the end)   median   spread    rounds"]
    med = {}
    for l in legs:
        med[l] = statistics.median(ms[l])
        lines.append(f"{what[l]}          {med[l]:8.4f} {max(ms[l]) - min(ms[l]):8.4f}    " + " ".join(f"{v:.4f}" for v in ms[l]))
    if "a" in med and "c" in med:
        lines.append(f"(c) - (a): {(med['c'] - med['a']) * 1e3:+.1f} us per step ({med['c'] / med['a']:.4f} x)")
    if "a" in med and "b" in med:
        lines.append(f"(b) - (a): {(med['b'] - med['a']) * 1e3:+.1f} us per step ({med['b'] / med['a']:.4f} x)")
    if metered is not None:
        m = metered["printed"][-1][1]
        lines.append("last (c) window: " + ", ".join(f"{k} avg {v.avg:.6g} n {v.count:g}" for k, v in m.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
