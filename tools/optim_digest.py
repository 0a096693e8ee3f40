#!/usr/bin/env python
"""Digests of everything the fused optimizers write (csrc/optim.hip), call by call: the yardstick for a change to the update
kernels or their host path that must leave every bit alone.  Drives FusedAdamW, FusedSGD and FusedLAMB through every update entry
of the library with seeded inputs generated on the CPU, and after every call prints a SHA-256 of every parameter, of both state
buffers, of the control block, of the returned norm and of the scaler's scale and growth tracker (and, where a schedule is
attached, of the schedule buffer).  Run it on the build before the change and on the build after it, on the same machine, and
compare the two outputs line by line; the digests pin one compiler's code generation, so they are a tool's output and not a test.

    python tools/optim_digest.py > digest.txt

The tensors: a sub-vector one, a tail-only one, sizes below, at and one past a chunk, a multi-chunk one with an n % 4 tail and a
2-d one, in two groups of which one has no weight decay.  ``misaligned``: one parameter and one gradient start 4 bytes into a
larger buffer (the scalar path).  One gradient is None in the second call (under accumulation: in the second cycle).
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import _lib as L  # noqa: E402
from mtlora_amd.lr_scheduler import CosineLRScheduler  # noqa: E402
from mtlora_amd.optim import FusedAdamW, FusedLAMB, FusedSGD, LossScaler  # noqa: E402

CHUNK = L.ADAMW_CHUNK
SHAPES = [(1,), (3,), (64,), (1023,), (CHUNK,), (CHUNK + 1,), (3 * CHUNK + 5,), (37, 129)]
MIS_P, MIS_G, NONE_G = 5, 6, 3  # the misaligned parameter, the misaligned gradient, the gradient that is None for a while
SCALE, MAX_NORM = 1024.0, 1.0


class AccumEntryAdamW(FusedAdamW):
    """FusedAdamW(capturable=True) that takes mtlora_adamw_accum_update_dev for every k (the class itself takes the plain entry at
    k = 1, so the accumulating entry's k = 1 form is out of its reach)"""

    def _launch(self, grad_ptrs, norm, max_norm, scaler_args, k):
        self.prepare_accumulation()
        self.push_hyperparameters()
        L.check(L.lib().mtlora_adamw_accum_update_dev(
            self._table.data_ptr(), grad_ptrs.data_ptr(), len(self._params), self._n_chunks, self._hyper_dev.data_ptr(),
            len(self.param_groups), max_norm, self._ctrl.data_ptr(), norm.data_ptr(), *scaler_args, self._scratch.data_ptr(),
            self._scratch_bytes, self._acc.data_ptr(), self._acc_offsets.data_ptr(), k, L.stream_ptr()), "adamw_accum_update_dev")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def offset_copy(t, dev):
    """a copy of ``t`` on ``dev`` that starts one element (4 bytes) into a larger buffer"""
    buf = torch.zeros(t.numel() + 1, device=dev)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def run(name, cls, kw, calls, k=1, misaligned=False, schedule=False, inf_at=None):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7)
    ps = []
    for i, s in enumerate(SHAPES):
        t = torch.randn(s, generator=gen) * 0.1
        ps.append(torch.nn.Parameter(offset_copy(t, dev) if misaligned and i == MIS_P else t.to(dev)))
    groups = [{"params": ps[0::2]}, {"params": ps[1::2], "weight_decay": 0.0}]
    opt = cls(groups, lr=1e-3, **kw)
    if schedule:
        opt.attach_schedule(CosineLRScheduler(opt, t_initial=6, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-6, t_in_epochs=False))
    scaler = LossScaler(init_scale=SCALE, growth_interval=2)
    tag = name + (" misaligned" if misaligned else "")
    for c in range(calls):
        for i, p in enumerate(ps):
            g = torch.randn(p.shape, generator=gen) * (1e-2 * SCALE)
            if c == inf_at and i == 2:
                g[0] = float("inf")
            p.grad = offset_copy(g, dev) if misaligned and i == MIS_G else g.to(dev)
        if c // k == 1:
            ps[NONE_G].grad = None
        norm = opt.clip_and_step(MAX_NORM, scaler, accumulation_steps=k)
        torch.cuda.synchronize()
        what = [(f"param{i}", p) for i, p in enumerate(ps)] + list(opt.state_tensors().items())
        what += [("norm", norm), ("scale", scaler._scale), ("tracker", scaler._growth_tracker)]
        for n, t in what:
            print(f"{sha(t)} {tag} call {c} {n}")


def main():
    for mis in (False, True):
        run("adamw", FusedAdamW, {}, 3, misaligned=mis)
        run("adamw dev", FusedAdamW, {"capturable": True}, 3, misaligned=mis)
        run("adamw accum k=3", FusedAdamW, {"capturable": True}, 6, k=3, misaligned=mis)
        run("sgd mu=0", FusedSGD, {"momentum": 0.0, "weight_decay": 1e-2}, 3, misaligned=mis)
        for cap in (False, True):
            d = " dev" if cap else ""
            run("sgd nesterov" + d, FusedSGD, {"momentum": 0.9, "nesterov": True, "weight_decay": 1e-2, "capturable": cap}, 3, misaligned=mis)
            run("lamb wd=0.01 nvlamb=0" + d, FusedLAMB, {"weight_decay": 0.01, "capturable": cap}, 3, misaligned=mis)
    # the entries and settings the loop above has not run, on the aligned layout
    run("adamw accum k=1", AccumEntryAdamW, {"capturable": True}, 2)
    run("adamw sched k=1", FusedAdamW, {"capturable": True}, 3, schedule=True)
    run("adamw sched k=2", FusedAdamW, {"capturable": True}, 4, k=2, schedule=True)
    run("sgd mu=0 dev", FusedSGD, {"momentum": 0.0, "weight_decay": 1e-2, "capturable": True}, 3)
    for cap in (False, True):
        d = " dev" if cap else ""
        run("sgd mu=0.9" + d, FusedSGD, {"momentum": 0.9, "weight_decay": 1e-2, "capturable": cap}, 3)
        for wd, nv in ((0.0, False), (0.0, True), (0.01, True)):
            run(f"lamb wd={wd} nvlamb={int(nv)}" + d, FusedLAMB, {"weight_decay": wd, "use_nvlamb": nv, "capturable": cap}, 3)
    for name, cls, kw in (("adamw", FusedAdamW, {}), ("sgd", FusedSGD, {"momentum": 0.9}), ("lamb", FusedLAMB, {})):
        run(name + " skipped", cls, kw, 2, inf_at=0)


if __name__ == "__main__":
    main()
