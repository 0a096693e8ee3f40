#!/usr/bin/env python
"""Generate tests/golden/eval_meters.pt by IMPORTING THE REAL REFERENCE meters and losses.

Run where a checkout of the reference (scale-lab/MTLoRA) is at hand:

    python tests/golden/make_golden_eval.py <path to the reference checkout>      (or MTLORA_REFERENCE=<path>)

Nothing from the reference is copied: the script imports the reference's ``evaluation/*`` (PerformanceMeter, get_output) and
``mtl_loss_schemes.get_loss``, feeds them small seeded full-resolution predictions and labels for all six
tasks in three batches, and records the inputs, the ``get_score()`` dicts, the per-batch loss values and one
``calculate_multi_task_performance`` value.  Modules that the meter FILES import at the top but the meter CLASSES never use
(``cv2``; the reference's own ``utils``, which drags in the training stack) are replaced by empty stand-ins if missing.

Inputs are stored as fp16 / uint8 so the file stays at about 100 kB; the recorded values were produced from exactly the
stored (rounded) inputs.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MTLORA_REFERENCE", "")
OUT = os.path.join(HERE, "eval_meters.pt")
TASKS = ["semseg", "human_parts", "normals", "sal", "depth", "edge"]
NCLS = {"semseg": 21, "human_parts": 7}
B, H, W, NB = 2, 16, 12, 3


def _shims():
    for name in ("cv2", "PIL", "PIL.Image", "scipy", "scipy.io"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    u = types.ModuleType("utils")  # eval_edge.py imports mkdir_if_missing from the reference's utils.py (never called by EdgeMeter)
    u.mkdir_if_missing = lambda d: os.makedirs(d, exist_ok=True)
    sys.modules["utils"] = u


def batch(i):
    """batch i: model outputs (B, C, H, W) and labels, rounded to the storage dtype"""
    g = torch.Generator().manual_seed(1000 + i)
    out, lab = {}, {}
    for t in ("semseg", "human_parts"):
        out[t] = (2 * torch.randn(B, NCLS[t], H, W, generator=g)).half().float()
        l = torch.randint(0, NCLS[t], (B, 1, H, W), generator=g).float()
        l[torch.rand(B, 1, H, W, generator=g) < 0.1] = 255.0
        # make the prediction right on about half of the pixels so that tp is not tiny
        hit = torch.rand(B, 1, H, W, generator=g) < 0.5
        boost = torch.zeros_like(out[t]).scatter_(1, l.clamp(max=NCLS[t] - 1).long(), 8.0)
        out[t] = torch.where(hit, out[t] + boost, out[t]).half().float()
        lab[t] = l
    out["normals"] = torch.randn(B, 3, H, W, generator=g).half().float()
    n = torch.nn.functional.normalize(out["normals"] + 0.7 * torch.randn(B, 3, H, W, generator=g), dim=1).half().float()
    ign = (torch.rand(B, 1, H, W, generator=g) < 0.1).expand(B, 3, H, W).clone()
    ign[:, 1:] |= torch.rand(B, 2, H, W, generator=g) < 0.02  # a few pixels with only SOME channels invalid (V1 != V2 masks)
    lab["normals"] = torch.where(ign, torch.full_like(n, 255.0), n)
    out["sal"] = (2 * torch.randn(B, 1, H, W, generator=g)).half().float()
    s = (torch.rand(B, 1, H, W, generator=g) < 0.3).float()
    s[0] = torch.where(out["sal"][0] > 0.5, torch.ones_like(s[0]), s[0] * (torch.rand(1, H, W, generator=g) < 0.3))
    if i == 1:
        s[1] = 0.0  # an image with no positive pixel ...
        out["sal"][1] = out["sal"][1].clamp(max=-3.0)  # ... and (nearly) nothing predicted: jaccard == 1 above sigmoid(-3) = 0.047
    s[torch.rand(B, 1, H, W, generator=g) < 0.03] = 255.0
    if i == 1:
        s[1] = 0.0
    lab["sal"] = s
    out["depth"] = (3 + 2 * torch.randn(B, 1, H, W, generator=g)).half().float()  # some values <= 0: the meter's clamp
    d = (0.5 + 9 * torch.rand(B, 1, H, W, generator=g)).half().float()
    d[torch.rand(B, 1, H, W, generator=g) < 0.1] = 255.0
    lab["depth"] = d
    out["edge"] = (2 * torch.randn(B, 1, H, W, generator=g) - 1).half().float()
    lab["edge"] = (torch.rand(B, 1, H, W, generator=g) < 0.1).float()
    return out, lab


def main():
    assert REF and os.path.isdir(REF), "pass the path of a reference checkout: golden vectors can only be regenerated from it"
    _shims()
    sys.path.insert(0, REF)
    from evaluation.evaluate_utils import PerformanceMeter, calculate_multi_task_performance, get_output
    from mtl_loss_schemes import get_loss

    cfg = types.SimpleNamespace(TASKS=TASKS)
    meter = PerformanceMeter(cfg, "PASCALContext")
    # (no meter.reset(): NormalsMeterV2 has no reset in the reference; a fresh meter starts at zero)
    crit = {t: get_loss({}, t) for t in TASKS}
    batches, losses = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(NB):
            out, lab = batch(i)
            losses.append({t: float(crit[t](out[t], lab[t])) for t in TASKS})
            meter.update({t: get_output(out[t], t) for t in TASKS}, {t: lab[t].clone() for t in TASKS})
            batches.append({"out": {t: v.half() for t, v in out.items()},
                            "lab": {t: (v.half() if t in ("normals", "depth") else v.to(torch.uint8)) for t, v in lab.items()}})
        scores = meter.get_score(verbose=False)
    scores = {t: {k: (list(map(float, v)) if isinstance(v, (list, tuple)) else float(v)) for k, v in d.items()}
              for t, d in scores.items()}
    # single-task stand-in scores for calculate_multi_task_performance (edge has no 'odsF' in its meter: left out there, as the
    # reference itself could not evaluate it)
    mt_tasks = [t for t in TASKS if t != "edge"]
    single = {t: {k: (v * 1.1 + 0.01 if not isinstance(v, list) else v) for k, v in scores[t].items()} for t in mt_tasks}
    mtp = float(calculate_multi_task_performance({t: scores[t] for t in mt_tasks}, single))
    torch.save({"tasks": TASKS, "batches": batches, "losses": losses, "scores": scores, "single": single,
                "multi_task_performance": mtp}, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    for t in TASKS:
        print(t, {k: v for k, v in scores[t].items() if k != "jaccards_all_categs"})


if __name__ == "__main__":
    main()
