"""Device-side batch ingest: the last stretch of the reference's loaders on the GPU.

Both reference pipelines (data/mtl_ds.py:838-870) end in ``AddIgnoreRegions -> ToTensor -> Normalize``
(data/custom_transforms.py:266-341), the training one starts with ``RandomHorizontalFlip`` (:192-209).  None of the four
resamples, so they can be reproduced bit for bit after the host-to-device copy -- which then carries the narrowest
lossless form of a batch instead of fp32 images and float64 labels (3.6 MB instead of 12.0 MB per 448 px image with the
four PASCAL tasks).

Wire format.  A host batch is a dict of contiguous CPU tensors (or numpy arrays), stacked over B:

    key                                  dtype, shape                 what it holds
    ``image``                            uint8 (B, H, W, 3)           the array ``ToTensor`` truncates with ``astype(np.uint8)``
                                                                      (custom_transforms.py:321), RGB
    ``semseg`` ``human_parts``           uint8 (B, H, W)              nearest-resized class maps, {0 .. C-1, 255}
    ``sal`` ``edge``                     uint8 (B, H, W)              binary maps, {0, 1} (255 = ignore passes through)
    ``normals``                          fp32 or fp16 (B, H, W, 3)    after ``FixedResize``'s renormalisation
    ``depth``                            fp32 (B, H, W)
    ``flip`` (optional)                  uint8 (B,)                   1 = mirror this sample

The synthetic tasks ``t0`` .. ``t7`` (mtl_harness.task_kind) use the normals format.  Semantics, per sample, in
this order -- ``prepare_batch_torch`` below is the definition, ``prepare_batch`` (csrc/ingest.hip) the implementation:

  1. flip, if flagged: mirror along W; normals channel 0 times -1 (RandomHorizontalFlip).
  2. AddIgnoreRegions: a normals pixel whose three components are all 0 becomes 255 in all three channels; a
     ``human_parts`` sample that is 0 everywhere becomes 255 everywhere; ``depth == 0`` becomes 255.
  3. ToTensor: image (B, 3, H, W) fp32 ``u8 / 255``; labels (B, C, H, W) fp32 (the reference: float64; every value here
     is an fp32 or narrower number, so fp32 holds it exactly -- the dtype train_step / validate_step take).
  4. Normalize: ``(x - mean[c]) / std[c]`` in fp32.

Resampling (ScaleNRotate, FixedResize) stays in the loader workers, on uint8 data.
"""
from __future__ import annotations

from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .mtl_harness import NUM_OUTPUT, task_kind

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # data/mtl_ds.py:861
IMAGENET_STD = (0.229, 0.224, 0.225)

_U8_KINDS = ("semseg", "human_parts", "sal", "edge")


def _as_tensor(x) -> torch.Tensor:
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(x)


def image_table(mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD) -> torch.Tensor:
    """the (3, 256) fp32 table of every value ``Normalize(ToTensor(u8))`` can take, built on the CPU with the operations
    torchvision's two transforms apply (``.to(float32).div(255)``, ``.sub_(mean).div_(std)`` with fp32 mean / std): the kernel
    looks pixels up in it, so the image is exact without an IEEE division on the device."""
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1)
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).view(1, 256)
    return ((v - m) / s).contiguous()


def check_wire_batch(batch: Mapping, tasks: Sequence[str]) -> Tuple[int, int, int]:
    """shapes and dtypes of a wire-format batch (see the module docstring); returns (B, H, W)"""
    if "image" not in batch:
        raise ValueError("wire batch: 'image' is missing")
    img = _as_tensor(batch["image"])
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError(f"wire batch: image must be uint8 (B, H, W, 3), got {img.dtype} {tuple(img.shape)}")
    B, H, W = img.shape[:3]
    for t in tasks:
        if t not in batch:
            raise ValueError(f"wire batch: task {t!r} is missing")
        x, k = _as_tensor(batch[t]), task_kind(t)
        if k in _U8_KINDS:
            ok = x.dtype == torch.uint8 and tuple(x.shape) == (B, H, W)
            want = "uint8 (B, H, W)"
        elif k == "normals":
            ok = x.dtype in (torch.float32, torch.float16) and tuple(x.shape) == (B, H, W, 3)
            want = "fp32 or fp16 (B, H, W, 3)"
        elif k == "depth":
            ok = x.dtype == torch.float32 and tuple(x.shape) == (B, H, W)
            want = "fp32 (B, H, W)"
        else:
            raise NotImplementedError(t)
        if not ok:
            raise ValueError(f"wire batch: {t} must be {want} with B, H, W = {(B, H, W)}, got {x.dtype} {tuple(x.shape)}")
    f = batch.get("flip")
    if f is not None:
        f = _as_tensor(f)
        if f.dtype != torch.uint8 or tuple(f.shape) != (B,):
            raise ValueError(f"wire batch: flip must be uint8 (B,), got {f.dtype} {tuple(f.shape)}")
    return B, H, W


def prepare_batch_torch(batch: Mapping, tasks: Sequence[str], mean: Sequence[float] = IMAGENET_MEAN,
                        std: Sequence[float] = IMAGENET_STD):
    """The semantics of the ingest, in plain torch on whatever device the batch lives on: ``(images, targets)`` as
    ``RandomHorizontalFlip`` (for the samples ``batch["flip"]`` flags), ``AddIgnoreRegions``, ``ToTensor`` and ``Normalize``
    give them, labels in fp32.  The documented definition and the tests' oracle; inputs are not modified."""
    B, H, W = check_wire_batch(batch, tasks)
    img = _as_tensor(batch["image"])
    dev = img.device
    flip = batch.get("flip")
    fl = None if flip is None else _as_tensor(flip).to(dev).bool()

    def mirrored(x):  # (B, H, W[, C]): flagged samples reversed along W
        return x if fl is None else torch.where(fl.view(B, *([1] * (x.dim() - 1))), x.flip(2), x)

    m = torch.as_tensor(mean, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    x = mirrored(img).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)  # ToTensor
    images = x.sub_(m).div_(s)                                                    # Normalize
    targets: Dict[str, torch.Tensor] = {}
    for t in tasks:
        k = task_kind(t)
        lab = mirrored(_as_tensor(batch[t]).to(dev))
        if k == "normals":
            lab = lab.to(torch.float32).clone()
            if fl is not None:
                lab[..., 0] = torch.where(fl.view(B, 1, 1), lab[..., 0] * -1, lab[..., 0])
            # AddIgnoreRegions tests sqrt(x^2 + y^2 + z^2) == 0 in float64.  For components that are fp32 (or fp16) numbers that
            # is "all three are 0": the square of the smallest fp32 denormal (2^-298) is a normal float64, so no term vanishes.
            ign = (lab == 0).all(dim=-1, keepdim=True)
            lab = torch.where(ign, torch.full_like(lab, 255.0), lab).permute(0, 3, 1, 2)
        elif k == "depth":
            lab = torch.where(lab == 0, torch.full_like(lab, 255.0), lab).unsqueeze(1)
        else:
            lab = lab.to(torch.float32)
            if k == "human_parts":
                empty = (lab == 0).flatten(1).all(dim=1).view(B, 1, 1)
                lab = torch.where(empty, torch.full_like(lab, 255.0), lab)
            lab = lab.unsqueeze(1)
        targets[t] = lab.contiguous()
    return images, targets


_tables: Dict[tuple, torch.Tensor] = {}


def _device_table(mean, std, device) -> torch.Tensor:
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), str(device))
    if key not in _tables:
        _tables[key] = image_table(mean, std).to(device)
    return _tables[key]


_JOB_KIND = {"semseg": "class", "sal": "class", "edge": "class", "human_parts": "class_allzero_ignore", "normals": "normals",
             "depth": "depth"}


def prepare_batch(batch: Mapping, tasks: Sequence[str], flip: Optional[torch.Tensor] = None,
                  mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD):
    """``prepare_batch_torch`` of a wire-format batch that already lives on the GPU, as ONE library call on the current stream
    (csrc/ingest.hip: at most three launches, no host sync).  ``flip``: uint8 (B,) on the device (default: ``batch["flip"]``
    if present, else no flips).  Returns ``(images, targets)``; GPU only, there is no CPU fallback."""
    from . import functional as Fn
    B, H, W = check_wire_batch(batch, tasks)
    img = batch["image"]
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise RuntimeError("mtlora_amd: prepare_batch takes a batch on a ROCm GPU (MI355X); the HIP path has no CPU fallback "
                           "(data.prepare_batch_torch is the portable restatement)")
    if flip is None:
        flip = batch.get("flip")
    if len(tasks) + 1 > L.INGEST_MAX_JOBS:
        raise RuntimeError(f"mtlora_amd: prepare_batch takes at most {L.INGEST_MAX_JOBS - 1} tasks per call")
    jobs = [("image", img)] + [(_JOB_KIND[task_kind(t)], batch[t]) for t in tasks]
    outs = Fn.ingest_batch(jobs, flip=flip, lut=_device_table(mean, std, img.device))
    return outs[0], dict(zip(tasks, outs[1:]))


def synthetic_wire_batch(B: int, S: int, tasks: Sequence[str], seed: int, num_outputs: Optional[Mapping[str, int]] = None,
                         normals_dtype: torch.dtype = torch.float32) -> Dict[str, torch.Tensor]:
    """a host batch in wire format with the label distributions of ``mtl_harness.synthetic_batch`` (class ids with 5 % 255, sal
    Bernoulli(.3), unit normals with 5 % ignored pixels, depth uniform in [0, 10), edge Bernoulli(.1)) and a uniform uint8
    image.  Ignored normals travel as (0, 0, 0), the value ``AddIgnoreRegions`` turns into 255."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = {"image": torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)}
    for t in tasks:
        k = task_kind(t)
        if k in ("semseg", "human_parts"):
            lab = torch.randint(0, int((num_outputs or {}).get(t, NUM_OUTPUT[k])), (B, S, S), generator=g, dtype=torch.uint8)
            lab[torch.rand(B, S, S, generator=g) < 0.05] = 255
        elif k == "sal":
            lab = (torch.rand(B, S, S, generator=g) < 0.3).to(torch.uint8)
        elif k == "normals":
            lab = torch.nn.functional.normalize(torch.randn(B, S, S, 3, generator=g), dim=-1)
            lab[torch.rand(B, S, S, generator=g) < 0.05] = 0.0
            lab = lab.to(normals_dtype)
        elif k == "depth":
            lab = torch.rand(B, S, S, generator=g) * 10
        elif k == "edge":
            lab = (torch.rand(B, S, S, generator=g) < 0.1).to(torch.uint8)
        else:
            raise NotImplementedError(t)
        out[t] = lab.contiguous()
    return out


class DeviceLoader:
    """Wraps any iterable of wire-format host batches and yields ``(images, targets)`` on ``device``, ready for
    ``train_step``, ``validate_step`` and ``predict``.

    A ring of ``depth`` pinned staging sets (host and device side) is filled ahead of the consumer: the host-to-device
    copies and ``prepare_batch`` of the next batches run on a side stream while the consumer works on the current one; an
    event makes the consumer's current stream wait for exactly the batch it receives.  The yielded tensors are fresh
    allocations, never part of the ring, and are marked (``record_stream``) as used on the consumer's stream, so they stay
    valid for as long as the consumer holds them.  A staging set is reused only after the ``prepare_batch`` that read it has
    finished (its event is waited for on the host before the pinned buffers are overwritten).  A host tensor that is
    already pinned (a ``DataLoader`` with ``pin_memory=True``) is copied from where it is and kept alive until then.

    ``flip_p``: probability of the horizontal flip per sample; the flags come from a host ``torch.Generator`` seeded with
    ``seed`` (one draw of B numbers per batch, in order), so a seed reproduces an epoch.  A ``flip`` entry in a host batch
    takes precedence.  GPU only."""

    def __init__(self, batches: Iterable[Mapping], tasks: Sequence[str], device, flip_p: float = 0.0, seed: int = 0,
                 depth: int = 2, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD):
        if not 0.0 <= float(flip_p) <= 1.0:
            raise ValueError(f"DeviceLoader: flip_p must be in [0, 1], got {flip_p}")
        if int(depth) != depth or depth < 1:
            raise ValueError(f"DeviceLoader: depth must be an integer >= 1, got {depth}")
        if len(tasks) == 0 or len(tasks) + 1 > L.INGEST_MAX_JOBS:
            raise ValueError(f"DeviceLoader: 1 to {L.INGEST_MAX_JOBS - 1} tasks, got {len(tasks)}")
        for t in tasks:
            if task_kind(t) not in _JOB_KIND:
                raise ValueError(f"DeviceLoader: unknown task {t!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mtlora_amd: DeviceLoader needs a ROCm GPU (MI355X) device; the HIP path has no CPU fallback")
        self.batches, self.tasks, self.device = batches, list(tasks), device
        self.flip_p, self.seed, self.depth = float(flip_p), int(seed), int(depth)
        self.mean, self.std = tuple(mean), tuple(std)
        self._stream = None
        self._ring = None

    def __len__(self):
        return len(self.batches)

    def _staging(self, slot: int, key: str, like: torch.Tensor, pinned: bool):
        """the device buffer of ring slot ``slot`` for ``key`` and, if asked for, its pinned host twin (re-made when the shape
        changes)"""
        cur = self._ring[slot]["buf"].get(key)
        if cur is None or cur[1].shape != like.shape or cur[1].dtype != like.dtype:
            cur = [None, torch.empty(like.shape, dtype=like.dtype, device=self.device)]
            self._ring[slot]["buf"][key] = cur
        if pinned and cur[0] is None:
            cur[0] = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
        return cur

    def _submit(self, slot: int, host: Mapping, gen: torch.Generator):
        keys = ["image"] + self.tasks
        B = check_wire_batch(host, self.tasks)[0]
        if host.get("flip") is not None:
            flip = _as_tensor(host["flip"])
        elif self.flip_p > 0.0:
            flip = (torch.rand(B, generator=gen) < self.flip_p).to(torch.uint8)
        else:
            flip = None
        entry = self._ring[slot]
        if entry["done"] is not None:
            entry["done"].synchronize()  # the ingest that read this slot's device buffers (and so its copies) has finished
        entry["hold"] = []
        dev_batch = {}
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            for k in keys + (["flip"] if flip is not None else []):
                src = flip if k == "flip" else _as_tensor(host[k])
                direct = src.is_pinned() and src.is_contiguous()  # (a DataLoader with pin_memory=True: copied from where it is)
                pinned, on_dev = self._staging(slot, k, src, pinned=not direct)
                if direct:
                    entry["hold"].append(src)  # alive until this slot's event has passed
                else:
                    pinned.copy_(src)
                on_dev.copy_(src if direct else pinned, non_blocking=True)
                dev_batch[k] = on_dev
            out = prepare_batch(dev_batch, self.tasks, mean=self.mean, std=self.std)
            entry["done"] = torch.cuda.Event()
            entry["done"].record(self._stream)
        return out, entry["done"], flip

    def __iter__(self):
        with torch.cuda.device(self.device):
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=self.device)
        self._ring = [{"buf": {}, "done": None, "hold": []} for _ in range(self.depth)]
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self.last_flips = []
        pending, slot = [], 0
        it = iter(self.batches)
        exhausted = False
        while True:
            while not exhausted and len(pending) < self.depth:
                try:
                    host = next(it)
                except StopIteration:
                    exhausted = True
                    break
                pending.append(self._submit(slot, host, gen))
                slot = (slot + 1) % self.depth
            if not pending:
                return
            (images, targets), done, flip = pending.pop(0)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(done)
            for t in [images] + list(targets.values()):
                t.record_stream(cur)
            self.last_flips.append(flip)
            yield images, targets
