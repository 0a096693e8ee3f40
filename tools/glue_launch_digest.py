#!/usr/bin/env python
"""Launch counts and gradient digests of ONE training step of the four-stage harness model (224 px, depths 2-2-2-2, batch 2):
the yardstick for a change to the autograd glue (mtlora_amd/functional.py) that must leave every launch and every bit of every
gradient alone.  Prints the library's per-kind launch counts of the step (mtlora_prof_begin / _end) and a SHA-256 of every
parameter gradient at fixed seeds; two runs of one tree that print different digests for a gradient show that this gradient is
not reproducible on that tree to begin with.

    python tools/glue_launch_digest.py [--img 224] [--batch 2]
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtlora_amd import _lib as L  # noqa: E402
from mtlora_amd import functional as Fn  # noqa: E402
from mtlora_amd import mtl_harness as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tasks = ["semseg", "normals", "sal", "human_parts"]
    torch.manual_seed(5)
    Fn._seed_counter = 0
    Fn.droppath_reset()
    model = H.build_model(img_size=a.img, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, seed=3).to(dev).train()
    crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3)
    img, tg = H.synthetic_batch(a.batch, a.img, tasks, seed=13, device=dev)
    torch.cuda.synchronize()
    lib = L.lib()
    L.check(lib.mtlora_prof_begin(400000), "prof_begin")
    loss, _ = H.train_step(model, crit, opt, img, tg, update_grad=False)  # forward + backward: the gradients stay
    torch.cuda.synchronize()
    s = L.ProfSummary()
    L.check(lib.mtlora_prof_end(ctypes.byref(s)), "prof_end")
    print(f"loss {loss.item()!r}")
    total = 0
    for k in range(L.PROF_KINDS):
        if s.count[k]:
            total += s.count[k]
            print(f"launches {lib.mtlora_prof_kind_name(k).decode():<16} {s.count[k]}")
    print(f"launches total            {total}")
    h_all = hashlib.sha256()
    n = 0
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        raw = p.grad.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        h_all.update(raw)
        n += 1
        print(f"grad {hashlib.sha256(raw).hexdigest()} {name}")
    print(f"grads {n} all {h_all.hexdigest()}")


if __name__ == "__main__":
    main()
