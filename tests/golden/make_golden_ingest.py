#!/usr/bin/env python
"""Generate tests/golden/ingest_tail.pt by IMPORTING THE REAL REFERENCE transforms.

Run where a checkout of the reference (scale-lab/MTLoRA) is at hand:

    python tests/golden/make_golden_ingest.py <path to the reference checkout>      (or MTLORA_REFERENCE=<path>)

Nothing from the reference is copied: the script loads the reference's ``data/custom_transforms.py`` and runs its real
``RandomHorizontalFlip``, ``AddIgnoreRegions``, ``ToTensor`` and ``Normalize`` classes, composed in the order of
data/mtl_ds.py:838-861, on small seeded samples (B = 2, 24 x 37, all six tasks), once per flip pattern, and records the
wire-format inputs next to the tensors the classes returned.

STUBS -- what ``custom_transforms.py`` imports at the top and a machine may lack is replaced ONLY as follows:
  * ``cv2``: one function, ``flip(a, flipCode=1)``, as a numpy mirror along axis 1 (a copy, as cv2 returns one).  Nothing else
    of cv2 is reachable from the four classes.
  * ``torchvision``: ``transforms.ToTensor`` and ``transforms.Normalize``, restated for the one input they get here: a uint8
    HWC array becomes ``torch.from_numpy(a.transpose(2, 0, 1)).contiguous().to(float32).div(255)``; Normalize clones and does
    ``sub_(mean[:, None, None]).div_(std[:, None, None])`` with fp32 mean / std.  A real torchvision is used if installed.
  * ``data.helpers``: an empty module (only FixedResize uses it).
``RandomHorizontalFlip`` draws ``numpy.random.random() < 0.5``; the script seeds numpy so that the draw comes out as the
pattern wants -- the class itself is not touched.

The reference works on float64 arrays (data/mtl_ds.py ``_load_*``: ``astype(float)``); the samples handed to it here are the
float64 widening of the stored fp32 / uint8 inputs (the image with a fractional part, which ``ToTensor`` truncates), so the
recorded float64 labels are exactly representable in fp32 -- asserted below -- and are stored as fp32.
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MTLORA_REFERENCE", "")
OUT = os.path.join(HERE, "ingest_tail.pt")
TASKS = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]
B, H, W = 2, 24, 37
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
FLIPS = [[0, 1], [1, 0]]  # every sample in both states


def _stubs():
    used = []
    try:
        importlib.import_module("cv2")
    except ImportError:
        cv2 = types.ModuleType("cv2")
        cv2.flip = lambda a, flipCode: np.ascontiguousarray(a[:, ::-1]) if flipCode == 1 else (_ for _ in ()).throw(NotImplementedError())
        for name in ("INTER_NEAREST", "INTER_CUBIC", "INTER_LINEAR"):
            setattr(cv2, name, name)
        sys.modules["cv2"] = cv2
        used.append("cv2.flip")
    try:
        importlib.import_module("torchvision")
    except ImportError:
        class ToTensor:
            def __call__(self, pic):
                assert isinstance(pic, np.ndarray) and pic.dtype == np.uint8 and pic.ndim == 3
                return torch.from_numpy(pic.transpose((2, 0, 1))).contiguous().to(dtype=torch.float32).div(255)

        class Normalize:
            def __init__(self, mean, std):
                self.mean, self.std = mean, std

            def __call__(self, t):
                t = t.clone()
                mean = torch.as_tensor(self.mean, dtype=t.dtype)
                std = torch.as_tensor(self.std, dtype=t.dtype)
                return t.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))

        tv, tf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tf.ToTensor, tf.Normalize, tv.transforms = ToTensor, Normalize, tf
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tf
        used.append("torchvision.transforms.ToTensor/Normalize")
    pkg, helpers = types.ModuleType("data"), types.ModuleType("data.helpers")
    pkg.helpers = helpers
    pkg.__path__ = []
    sys.modules["data"], sys.modules["data.helpers"] = pkg, helpers
    used.append("data.helpers")
    return used


def wire_inputs():
    g = torch.Generator().manual_seed(20240)
    img = torch.rand(B, H, W, 3, generator=g) * 255.99  # what ToTensor truncates
    img[0, 0, 0] = torch.tensor([0.0, 255.0, 254.999])
    wire = {"image": img.to(torch.uint8)}
    sem = torch.randint(0, 21, (B, H, W), generator=g, dtype=torch.uint8)
    sem[torch.rand(B, H, W, generator=g) < 0.1] = 255
    hp = torch.randint(0, 7, (B, H, W), generator=g, dtype=torch.uint8)
    hp[torch.rand(B, H, W, generator=g) < 0.1] = 255
    hp[0] = 0  # a sample without human part annotations
    wire.update(semseg=sem, human_parts=hp, sal=(torch.rand(B, H, W, generator=g) < 0.3).to(torch.uint8),
                edge=(torch.rand(B, H, W, generator=g) < 0.1).to(torch.uint8))
    nrm = torch.nn.functional.normalize(torch.randn(B, H, W, 3, generator=g), dim=-1)
    nrm[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    nrm[0, 1, 2] = torch.tensor([-0.0, 0.0, -0.0])
    nrm[1, 3, 36] = torch.tensor([0.0, 0.6, 0.8])     # a zero first component on the last column
    nrm[1, 5, 0] = torch.tensor([1e-45, 0.0, 0.0])    # the smallest fp32 denormal: not an ignore pixel
    dep = torch.rand(B, H, W, generator=g) * 10
    dep[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    wire.update(normals=nrm, depth=dep)
    return img, wire


def seed_for(flip: bool) -> int:
    """a numpy seed whose first ``random()`` draw makes RandomHorizontalFlip flip (or not)"""
    s = 0
    while (np.random.RandomState(s).random_sample() < 0.5) != flip:
        s += 1
    return s


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit(__doc__)
    used = _stubs()
    spec = importlib.util.spec_from_file_location("ref_custom_transforms", os.path.join(REF, "data", "custom_transforms.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    tail = [tr.AddIgnoreRegions(), tr.ToTensor(), tr.Normalize(MEAN, STD)]
    img, wire = wire_inputs()
    rec = {"tasks": TASKS, "mean": MEAN, "std": STD, "wire": wire, "flips": FLIPS, "outputs": [], "stubs": used}
    for pattern in FLIPS:
        outs = []
        for b in range(B):
            sample = {"image": img[b].double().numpy().copy()}
            for t in TASKS:
                sample[t] = wire[t][b].double().numpy().copy()
            np.random.seed(seed_for(bool(pattern[b])))
            sample = tr.RandomHorizontalFlip()(sample)
            for f in tail:
                sample = f(sample)
            outs.append(sample)
        stacked = {}
        for k in ["image"] + TASKS:
            v = torch.stack([o[k] for o in outs])
            if k != "image":
                assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), k
                v = v.float()
            assert v.dtype == torch.float32
            stacked[k] = v
        rec["outputs"].append(stacked)
    torch.save(rec, OUT)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; stubs: {used}")


if __name__ == "__main__":
    main()
