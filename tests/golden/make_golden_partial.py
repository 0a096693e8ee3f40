#!/usr/bin/env python
"""Generate tests/golden/partial_labels.pt by IMPORTING THE REAL REFERENCE losses.

Run where a checkout of the reference (scale-lab/MTLoRA) is at hand:

    python tests/golden/make_golden_partial.py <path to the reference checkout>      (or MTLORA_REFERENCE=<path>)

Nothing from the reference is copied: the script imports the reference's ``mtl_loss_schemes.get_loss``, and for each of the six
tasks and each per-sample validity mask applies the task's criterion IN FP64 to the index-selected sub-batch
``(pred[V], gt[V])`` of one seeded full-resolution batch (B = 3, 16 x 16), which is what a partially labelled batch means in
this project.  Recorded: the inputs, the loss values (Python floats, fp64) and a compact form of
``g = d loss / d pred[V]``: its K = 8 projections ``<g, P_k>`` onto the fixed +-1 patterns of ``probes()`` below (fp64), its
Euclidean norm and its largest magnitude.  A gradient that differs from g by d moves projection k by ``<d, P_k>``, of the order
of ``|d|_2``: eight of them do not all vanish for a d that matters.

The all-zero mask is not recorded: the reference divides by zero there.  Inputs are stored as fp16 / uint8, semseg with 6 and
human_parts with 4 classes (the criterion does not know the number), so the file stays at about 35 kB; the recorded values were
produced from exactly the stored (rounded) inputs.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MTLORA_REFERENCE", "")
OUT = os.path.join(HERE, "partial_labels.pt")
TASKS = ["semseg", "human_parts", "normals", "sal", "depth", "edge"]
NCLS = {"semseg": 6, "human_parts": 4}
K = 8
MASKS = [[1, 1, 1], [1, 0, 1], [0, 0, 1]]
B, H, W = 3, 16, 16


def probes(n, k=K):
    """(k, n) float64 patterns of +-1 from integer arithmetic alone (no random generator: the same on every torch version)"""
    i = torch.arange(n, dtype=torch.int64).view(1, n)
    j = torch.arange(k, dtype=torch.int64).view(k, 1)
    h = (i * 2654435761 + (j + 1) * 40503 + (i >> 5) * (2 * j + 7) * 97) % (1 << 32)
    h = (h ^ (h >> 13)) * 1274126177 % (1 << 32)
    return (((h >> 15) & 1) * 2 - 1).to(torch.float64)


def compact(g):
    """the recorded form of a gradient: projections, Euclidean norm, largest magnitude"""
    g = g.detach().double().reshape(-1)
    return {"proj": (probes(g.numel()) @ g).tolist(), "l2": float(g.norm()), "max": float(g.abs().max())}


def batch():
    """model outputs (B, C, H, W) and labels, rounded to the storage dtype"""
    g = torch.Generator().manual_seed(2024)
    out, lab = {}, {}
    for t in ("semseg", "human_parts"):
        out[t] = (2 * torch.randn(B, NCLS[t], H, W, generator=g)).half().float()
        l = torch.randint(0, NCLS[t], (B, 1, H, W), generator=g).float()
        l[torch.rand(B, 1, H, W, generator=g) < 0.1] = 255.0
        lab[t] = l
    out["normals"] = torch.randn(B, 3, H, W, generator=g).half().float()
    n = torch.nn.functional.normalize(out["normals"] + 0.7 * torch.randn(B, 3, H, W, generator=g), dim=1).half().float()
    ign = (torch.rand(B, 1, H, W, generator=g) < 0.1).expand(B, 3, H, W).clone()
    lab["normals"] = torch.where(ign, torch.full_like(n, 255.0), n)
    out["sal"] = (2 * torch.randn(B, 1, H, W, generator=g)).half().float()
    # a different share of positives per sample, so that w depends on which samples are labelled
    lab["sal"] = (torch.rand(B, 1, H, W, generator=g) < torch.tensor([0.15, 0.3, 0.6]).view(B, 1, 1, 1)).float()
    out["depth"] = (3 + 2 * torch.randn(B, 1, H, W, generator=g)).half().float()
    d = (0.5 + 9 * torch.rand(B, 1, H, W, generator=g)).half().float()
    d[torch.rand(B, 1, H, W, generator=g) < 0.1] = 255.0
    lab["depth"] = d
    out["edge"] = (2 * torch.randn(B, 1, H, W, generator=g) - 1).half().float()
    lab["edge"] = (torch.rand(B, 1, H, W, generator=g) < 0.1).float()
    return out, lab


def main():
    assert REF and os.path.isdir(REF), "pass the path of a reference checkout: golden vectors can only be regenerated from it"
    sys.path.insert(0, REF)
    from mtl_loss_schemes import get_loss

    crit = {t: get_loss({}, t) for t in TASKS}
    out, lab = batch()
    cases = []
    for mask in MASKS:
        idx = torch.tensor([b for b in range(B) if mask[b]])
        loss, grad = {}, {}
        for t in TASKS:
            p = out[t].double().index_select(0, idx).requires_grad_(True)
            v = crit[t](p, lab[t].double().index_select(0, idx))
            assert v.dtype == torch.float64
            v.backward()
            loss[t], grad[t] = float(v.detach()), compact(p.grad)
        cases.append({"mask": mask, "loss": loss, "grad": grad})
    torch.save({"tasks": TASKS, "out": {t: v.half() for t, v in out.items()},
                "lab": {t: (v.half() if t in ("normals", "depth") else v.to(torch.uint8)) for t, v in lab.items()},
                "cases": cases}, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    for c in cases:
        print(c["mask"], c["loss"])


if __name__ == "__main__":
    main()
