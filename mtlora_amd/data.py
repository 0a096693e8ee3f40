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
    ``valid`` (optional)                 {task: uint8 (B,)}           non-zero = the sample carries a label for that task; a task
                                                                      without an entry is labelled everywhere

The synthetic tasks ``t0`` .. ``t7`` (mtl_harness.task_kind) use the normals format.  Semantics, per sample, in
this order -- ``prepare_batch_torch`` below is the definition, ``prepare_batch`` (csrc/ingest.hip) the implementation:

  1. flip, if flagged: mirror along W; normals channel 0 times -1 (RandomHorizontalFlip).
  2. AddIgnoreRegions: a normals pixel whose three components are all 0 becomes 255 in all three channels; a
     ``human_parts`` sample that is 0 everywhere becomes 255 everywhere; ``depth == 0`` becomes 255.
  3. ToTensor: image (B, 3, H, W) fp32 ``u8 / 255``; labels (B, C, H, W) fp32 (the reference: float64; every value here
     is an fp32 or narrower number, so fp32 holds it exactly -- the dtype train_step / validate_step take).
  4. Normalize: ``(x - mean[c]) / std[c]`` in fp32.

Partially labelled batches.  With ``valid``, the label plane of a sample flagged 0 still travels and is still ingested (the
kernels walk whole tensors), but its content is undefined, on the wire and after the ingest: the fused losses never read it
(``functional.UpsampleLossFn``).  ``prepare_batch`` / ``prepare_batch_torch`` / ``DeviceLoader`` hand the flags through as a third
value, ``(images, targets, valid)``, only when the batch carries them.  ``merge_wire_batches`` builds such a batch from two
datasets with different task sets (PASCAL-Context + NYUD).  The flip does not touch the flags (they are per sample).

Resampling (ScaleNRotate, FixedResize) runs on the device as well, in front of the ingest: the loader workers ship the
decoded, un-resampled sample and the GPU produces the wire-format batch above.

Raw batch ("canvas format", ``check_raw_batch``).  The same keys and dtypes as the wire format (normals fp32 only), every
tensor stacked on a common canvas ``(B, Hc, Wc[, 3])``, plus ``size``: int32 (B, 2), each sample's ``(h, w)`` with
``1 <= h <= Hc``, ``1 <= w <= Wc``.  Sample b occupies the top-left ``h x w`` rectangle of its canvas; canvas pixels outside it are
never read and count as border.  Optional ``flip`` as above, ``rot_deg`` and ``scale`` (float (B,)) for ``DeviceLoader``.

Augmentation semantics -- ``augment_batch_torch`` is the definition, ``augment_batch`` (csrc/augment.hip) the implementation.
Per sample, ``make_geometry`` (host, float64) composes the inverse of ``cv2.getRotationMatrix2D((w / 2, h / 2), rot, sc)``
(custom_transforms.py:60-63; warpAffine's convention: integer coordinates are pixel centres, no half-pixel shift) with
``FixedResize``'s pixel-centre map ``xi = (u + 0.5) w / Wo - 0.5`` and rounds the result to ``GEOM_BITS`` = 24 fraction bits:
the source coordinate of output pixel (u, v) is ``X = ax (2u + 1) + bx (2v + 1) + cx`` (``Y`` likewise) in int64.  From there
all coordinate arithmetic is integer, here and in the kernel, which is what makes the two agree bit for bit:

  * nearest (every uint8 label map, and depth; ``FLAGVALS``, mtl_ds.py:754-803): ``(X + 2^23) >> 24``, round half up with an
    arithmetic shift.  Outside ``[0, w) x [0, h)`` the result is 0 (cv2's ``BORDER_CONSTANT`` 0; ``AddIgnoreRegions`` then turns a
    0 normal or a 0 depth into 255, as in the reference).
  * cubic (image, normals): ``(X + 2^18) >> 19`` is the coordinate in 1/32 pixel (cv2's ``INTER_BITS``), ``>> 5`` its integer
    part, ``& 31`` the fraction f.  4 x 4 taps, a tap outside the rectangle contributes 0, weights ``cubic_table()[f]`` (Keys,
    a = -0.75, cv2's ``INTER_CUBIC``).  uint8 image: Q15 weights, exact integer accumulation, ``clamp((acc + 2^29) >> 30, 0, 255)``.
    fp32 normals: fp32 multiplies and adds in a fixed order, horizontal first (left to right), then vertical (top to bottom).
  * normals, after the interpolation: the in-plane rotation of custom_transforms.py:74-80 as the 2 x 2 rotation it is,
    ``x' = x cos + y sin``, ``y' = y cos - x sin`` with the fp32 values of the side table; then ``FixedResize``'s renormalisation
    ``n / (|n| + NORMALS_EPS)`` (:144-150).  A pixel whose three components are all 0 stays 0.
  * depth: the nearest sample divided by ``sc`` (:83-84).

Deviations from the reference, on purpose.  (1) ONE resample where the reference has two (it warps at source size, then
resizes).  (2) The flip stays where the ingest applies it, after the warp; that equals the reference's flip-then-warp in
distribution, up to the half pixel between ``w / 2`` and ``(w - 1) / 2``.  (3) The random numbers come from the loader's
``torch.Generator``, not from ``numpy.random``.  (4) No fixture can be generated from the reference for this stage (cv2 is not
available where the fixtures are made): the tests anchor the definition to cv2's documented conventions, they are not a cv2
parity claim.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Mapping, NamedTuple, Optional, Sequence, Tuple

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


def _check_valid(batch: Mapping, tasks: Sequence[str], B: int, what: str) -> None:
    v = batch.get("valid")
    if v is None:
        return
    if not isinstance(v, Mapping):
        raise ValueError(f"{what}: valid must be a dict {{task: uint8 (B,)}}, got {type(v).__name__}")
    for t, x in v.items():
        if t not in tasks:
            raise ValueError(f"{what}: valid names {t!r}, which is not one of the tasks {list(tasks)}")
        x = _as_tensor(x)
        if x.dtype != torch.uint8 or tuple(x.shape) != (B,):
            raise ValueError(f"{what}: valid[{t!r}] must be uint8 (B,) with B = {B}, got {x.dtype} {tuple(x.shape)}")


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
    _check_valid(batch, tasks, B, "wire batch")
    return B, H, W


def prepare_batch_torch(batch: Mapping, tasks: Sequence[str], mean: Sequence[float] = IMAGENET_MEAN,
                        std: Sequence[float] = IMAGENET_STD):
    """The semantics of the ingest, in plain torch on whatever device the batch lives on: ``(images, targets)`` as
    ``RandomHorizontalFlip`` (for the samples ``batch["flip"]`` flags), ``AddIgnoreRegions``, ``ToTensor`` and ``Normalize``
    give them, labels in fp32.  The documented definition and the tests' oracle; inputs are not modified.  A batch with
    ``valid`` returns ``(images, targets, valid)``, the flags as uint8 tensors on the batch's device."""
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
    if batch.get("valid") is not None:
        return images, targets, {t: _as_tensor(v).to(dev) for t, v in batch["valid"].items()}
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
    if present, else no flips).  Returns ``(images, targets)`` -- ``(images, targets, valid)`` for a batch with ``valid``, the flags as
    uint8 tensors on the device --; GPU only, there is no CPU fallback."""
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
    if batch.get("valid") is not None:
        return outs[0], dict(zip(tasks, outs[1:])), {t: _as_tensor(v).to(img.device) for t, v in batch["valid"].items()}
    return outs[0], dict(zip(tasks, outs[1:]))


def merge_wire_batches(a: Mapping, tasks_a: Sequence[str], b: Mapping, tasks_b: Sequence[str]):
    """One wire batch over the union of two task sets from two wire batches of the same image size (a PASCAL-Context batch and
    an NYUD batch): the samples of ``a`` first, then those of ``b``.  A task that only one side has gets a label plane for the
    other side's samples that is allocated and NOT defined (``torch.empty``), and ``valid[task]`` flags those samples 0; a task
    both sides have is labelled everywhere (flags given by either side are kept).  ``flip`` is concatenated when either side has
    one (0 for the other).  Returns ``(batch, tasks)``, the union in the order of ``tasks_a``, then the new ones of ``tasks_b``.
    Host or device tensors, both batches on the same device."""
    Ba, H, W = check_wire_batch(a, tasks_a)
    Bb, Hb, Wb = check_wire_batch(b, tasks_b)
    if (H, W) != (Hb, Wb):
        raise ValueError(f"merge_wire_batches: image sizes differ, {(H, W)} and {(Hb, Wb)}")
    tasks = list(tasks_a) + [t for t in tasks_b if t not in tasks_a]
    ia, ib = _as_tensor(a["image"]), _as_tensor(b["image"])
    out = {"image": torch.cat([ia, ib], 0)}
    dev = ia.device
    va, vb = a.get("valid") or {}, b.get("valid") or {}
    valid = {}
    for t in tasks:
        xa = _as_tensor(a[t]) if t in tasks_a else None
        xb = _as_tensor(b[t]) if t in tasks_b else None
        if xa is not None and xb is not None and xa.dtype != xb.dtype:  # (normals: fp32 on one side, fp16 on the other)
            xa, xb = xa.to(torch.float32), xb.to(torch.float32)
        if xa is None:
            xa = torch.empty((Ba,) + tuple(xb.shape[1:]), dtype=xb.dtype, device=dev)
        if xb is None:
            xb = torch.empty((Bb,) + tuple(xa.shape[1:]), dtype=xa.dtype, device=dev)
        out[t] = torch.cat([xa, xb], 0)
        fa = _as_tensor(va[t]).to(dev) if t in va else torch.full((Ba,), int(t in tasks_a), dtype=torch.uint8, device=dev)
        fb = _as_tensor(vb[t]).to(dev) if t in vb else torch.full((Bb,), int(t in tasks_b), dtype=torch.uint8, device=dev)
        valid[t] = torch.cat([fa, fb], 0)
    out["valid"] = valid
    if a.get("flip") is not None or b.get("flip") is not None:
        fl = [(_as_tensor(x["flip"]).to(dev) if x.get("flip") is not None else torch.zeros(n, dtype=torch.uint8, device=dev))
              for x, n in ((a, Ba), (b, Bb))]
        out["flip"] = torch.cat(fl, 0)
    return out, tasks


def synthetic_wire_batch(B: int, S: int, tasks: Sequence[str], seed: int, num_outputs: Optional[Mapping[str, int]] = None,
                         normals_dtype: torch.dtype = torch.float32,
                         valid: Optional[Mapping[str, Sequence[int]]] = None) -> Dict[str, torch.Tensor]:
    """a host batch in wire format with the label distributions of ``mtl_harness.synthetic_batch`` (class ids with 5 % 255, sal
    Bernoulli(.3), unit normals with 5 % ignored pixels, depth uniform in [0, 10), edge Bernoulli(.1)) and a uniform uint8
    image.  Ignored normals travel as (0, 0, 0), the value ``AddIgnoreRegions`` turns into 255.  ``valid`` (``{task: B flags}``):
    the batch carries these flags, and the label planes of the samples flagged 0 are overwritten with garbage (NaN for normals
    and depth, 0xFF bytes for the uint8 maps); the labelled samples and the random draws are those of the call without it."""
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
        if valid is not None and t in valid:
            lab[torch.as_tensor(valid[t]).reshape(B) == 0] = 255 if lab.dtype == torch.uint8 else float("nan")
        out[t] = lab.contiguous()
    if valid is not None:
        out["valid"] = {t: torch.as_tensor(v).reshape(B).ne(0).to(torch.uint8) for t, v in valid.items()}
    return out


# ----------------------------------------------------------------------------------------------
# geometric augmentation (ScaleNRotate + FixedResize) in front of the ingest
# ----------------------------------------------------------------------------------------------
GEOM_BITS = L.AUGMENT_GEOM_BITS              # fraction bits of the fixed-point geometry
NORMALS_EPS = 2.220446049250313e-16          # np.finfo(float).eps of FixedResize's renormalisation; 2^-52, an fp32 number too

_AUG_KIND = {"semseg": "class_nearest_u8", "human_parts": "class_nearest_u8", "sal": "class_nearest_u8", "edge": "class_nearest_u8",
             "normals": "normals_cubic_f32", "depth": "depth_nearest_f32"}


class Geometry(NamedTuple):
    """what ``make_geometry`` returns: ``coef`` int64 (B, 6) = ax, bx, cx, ay, by, cy with ``GEOM_BITS`` fraction bits, ``side``
    fp32 (B, 3) = cos(rot), sin(rot), sc"""
    coef: torch.Tensor
    side: torch.Tensor


def check_raw_batch(batch: Mapping, tasks: Sequence[str]) -> Tuple[int, int, int]:
    """shapes, dtypes and sizes of a raw (canvas-format) batch (see the module docstring); returns (B, Hc, Wc).  The values of
    ``size`` are checked when it lives on the host (on the device the kernel clamps them to the canvas)."""
    if "image" not in batch:
        raise ValueError("raw batch: 'image' is missing")
    img = _as_tensor(batch["image"])
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError(f"raw batch: image must be uint8 (B, Hc, Wc, 3), got {img.dtype} {tuple(img.shape)}")
    B, Hc, Wc = img.shape[:3]
    if B < 1 or Hc < 1 or Wc < 1:
        raise ValueError(f"raw batch: empty canvas {tuple(img.shape)}")
    for t in tasks:
        if t not in batch:
            raise ValueError(f"raw batch: task {t!r} is missing")
        x, k = _as_tensor(batch[t]), task_kind(t)
        if k in _U8_KINDS:
            ok, want = x.dtype == torch.uint8 and tuple(x.shape) == (B, Hc, Wc), "uint8 (B, Hc, Wc)"
        elif k == "normals":
            ok, want = x.dtype == torch.float32 and tuple(x.shape) == (B, Hc, Wc, 3), "fp32 (B, Hc, Wc, 3)"
        elif k == "depth":
            ok, want = x.dtype == torch.float32 and tuple(x.shape) == (B, Hc, Wc), "fp32 (B, Hc, Wc)"
        else:
            raise NotImplementedError(t)
        if not ok:
            raise ValueError(f"raw batch: {t} must be {want} with B, Hc, Wc = {(B, Hc, Wc)}, got {x.dtype} {tuple(x.shape)}")
    if "size" not in batch:
        raise ValueError("raw batch: 'size' is missing")
    size = _as_tensor(batch["size"])
    if size.dtype != torch.int32 or tuple(size.shape) != (B, 2):
        raise ValueError(f"raw batch: size must be int32 (B, 2), got {size.dtype} {tuple(size.shape)}")
    if not size.is_cuda:
        h, w = size[:, 0], size[:, 1]
        if bool((h < 1).any()) or bool((h > Hc).any()) or bool((w < 1).any()) or bool((w > Wc).any()):
            raise ValueError(f"raw batch: size must hold 1 <= h <= {Hc} and 1 <= w <= {Wc}, got {size.tolist()}")
    f = batch.get("flip")
    if f is not None:
        f = _as_tensor(f)
        if f.dtype != torch.uint8 or tuple(f.shape) != (B,):
            raise ValueError(f"raw batch: flip must be uint8 (B,), got {f.dtype} {tuple(f.shape)}")
    return B, Hc, Wc


def _out_size(out_size) -> Tuple[int, int]:
    try:
        Ho, Wo = out_size
        ok = int(Ho) == Ho and int(Wo) == Wo and Ho >= 1 and Wo >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"out_size must be two integers (Ho, Wo) >= 1, got {out_size!r}")
    return int(Ho), int(Wo)


def make_geometry(size, rot_deg, scale, out_size) -> Geometry:
    """The per-sample map from output pixels to source coordinates, composed on the host in float64 and rounded ONCE to
    fixed point.  ``size``: (B, 2) integers (h, w); ``rot_deg``, ``scale``: (B,) numbers (or scalars); ``out_size``: (Ho, Wo).

    ``cv2.getRotationMatrix2D((w / 2, h / 2), rot, sc)`` maps source to destination by ``d - c = sc R (s - c)``; warpAffine reads
    ``s = c + R^T (d - c) / sc`` for every destination pixel d, and ``FixedResize`` reads that destination at
    ``d = ((u + 0.5) w / Wo - 0.5, (v + 0.5) h / Ho - 0.5)``.  With C = cos(rot), S = sin(rot):

        xs = cx + ( C (xd - cx) - S (yd - cy)) / sc  =  ax (2u + 1) + bx (2v + 1) + cx'
        ys = cy + ( S (xd - cx) + C (yd - cy)) / sc  =  ay (2u + 1) + by (2v + 1) + cy'

    C and S are exact for multiples of 90 degrees.  Returns ``Geometry(coef, side)``."""
    Ho, Wo = _out_size(out_size)
    size = torch.as_tensor(size).to(torch.float64).reshape(-1, 2)
    B = size.shape[0]
    rot = torch.as_tensor(rot_deg, dtype=torch.float64).reshape(-1).expand(B).clone()
    sc = torch.as_tensor(scale, dtype=torch.float64).reshape(-1).expand(B).clone()
    if bool((size < 1).any()):
        raise ValueError(f"make_geometry: sizes must be >= 1, got {size.tolist()}")
    if not bool(torch.isfinite(rot).all()) or not bool(torch.isfinite(sc).all()) or bool((sc <= 0).any()):
        raise ValueError("make_geometry: rot_deg must be finite and scale finite and > 0")
    h, w = size[:, 0], size[:, 1]
    C, S = torch.cos(torch.deg2rad(rot)), torch.sin(torch.deg2rad(rot))
    q = rot / 90.0
    exact = q == q.round()
    k = q.round().to(torch.int64) % 4
    C = torch.where(exact, torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=torch.float64)[k], C)
    S = torch.where(exact, torch.tensor([0.0, 1.0, 0.0, -1.0], dtype=torch.float64)[k], S)
    cx, cy = w / 2, h / 2
    ax, bx = C * w / (2 * Wo * sc), -S * h / (2 * Ho * sc)
    ay, by = S * w / (2 * Wo * sc), C * h / (2 * Ho * sc)
    c0 = cx + (-C * (0.5 + cx) + S * (0.5 + cy)) / sc
    c1 = cy + (-S * (0.5 + cx) - C * (0.5 + cy)) / sc
    real = torch.stack([ax, bx, c0, ay, by, c1], dim=1)
    reach = (real[:, [0, 3]].abs() * (2 * Wo) + real[:, [1, 4]].abs() * (2 * Ho) + real[:, [2, 5]].abs()).max()
    if float(reach) >= 2.0 ** (61 - GEOM_BITS):
        raise ValueError("make_geometry: source coordinates out of the fixed-point range (scale too small for this size)")
    coef = torch.round(real * float(1 << GEOM_BITS)).to(torch.int64)
    side = torch.stack([C, S, sc], dim=1).to(torch.float32)
    return Geometry(coef.contiguous(), side.contiguous())


_cubic = None


def cubic_table() -> Tuple[torch.Tensor, torch.Tensor]:
    """the four cubic weights (Keys kernel, a = -0.75: cv2's INTER_CUBIC, ``interpolateCubic``) of the taps at -1, 0, 1, 2 for
    the fractions t = f / 32, f = 0 .. 31, as ``(q15, f32)``: int32 (32, 4) in Q15 with every row summing to exactly 32768 (the
    rounding correction on the row's largest weight) and fp32 (32, 4) = q15 / 32768.  The fp32 form is the Q15 form on
    purpose: 16-bit numbers add exactly in fp32 in any order, so its rows sum to exactly 1.0 however they are added -- a
    constant image or normal map stays constant -- and both forms are symmetric under t <-> 1 - t.  Built once on the host."""
    global _cubic
    if _cubic is None:
        A = -0.75
        t = torch.arange(32, dtype=torch.float64) / 32
        w = torch.stack([((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                         ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1], dim=1)
        w = torch.cat([w, 1 - w.sum(1, keepdim=True)], dim=1)
        q = torch.round(w * 32768).to(torch.int64)
        rows = torch.arange(32)
        # the largest weight is tap 0's for t <= 1/2 and tap 1's beyond: first-largest below the middle, last-largest above it, so
        # that row 32 - f stays the mirror image of row f
        big = torch.where(rows <= 16, q.argmax(1), 3 - q.flip(1).argmax(1))
        q[rows, big] += 32768 - q.sum(1)
        assert bool((q.sum(1) == 32768).all())
        _cubic = (q.to(torch.int32).contiguous(), (q.to(torch.float32) / 32768).contiguous())
    return _cubic


def _nearest_index(X, Y, h, w, Wc):
    half = 1 << (GEOM_BITS - 1)
    xn, yn = (X + half) >> GEOM_BITS, (Y + half) >> GEOM_BITS
    inside = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    return (yn.clamp(min=0) * Wc + xn.clamp(min=0)) * inside, inside  # (index 0 where outside: read but not used)


def augment_batch_torch(raw: Mapping, tasks: Sequence[str], geom: Geometry, out_size, renormalize: bool = True):
    """The semantics of the device-side ``ScaleNRotate`` + ``FixedResize`` (see the module docstring), in plain torch on whatever
    device the batch lives on: a raw canvas-format batch and its ``make_geometry`` in, the wire-format batch at ``out_size``
    out (``flip`` passes through).  The documented definition and the tests' oracle; inputs are not modified.
    ``renormalize=False`` returns the normals as the interpolation and the in-plane rotation leave them."""
    B, Hc, Wc = check_raw_batch(raw, tasks)
    Ho, Wo = _out_size(out_size)
    img = _as_tensor(raw["image"])
    dev = img.device
    coef, side = _as_tensor(geom.coef).to(dev), _as_tensor(geom.side).to(dev)
    if coef.dtype != torch.int64 or tuple(coef.shape) != (B, 6) or side.dtype != torch.float32 or tuple(side.shape) != (B, 3):
        raise ValueError("augment: geom must be make_geometry's (int64 (B, 6), fp32 (B, 3))")
    size = _as_tensor(raw["size"]).to(dev).to(torch.int64)
    h, w = size[:, 0].clamp(0, Hc).view(B, 1, 1), size[:, 1].clamp(0, Wc).view(B, 1, 1)
    u2 = (2 * torch.arange(Wo, dtype=torch.int64, device=dev) + 1).view(1, 1, Wo)
    v2 = (2 * torch.arange(Ho, dtype=torch.int64, device=dev) + 1).view(1, Ho, 1)
    c = [coef[:, i].view(B, 1, 1) for i in range(6)]
    X, Y = c[0] * u2 + c[1] * v2 + c[2], c[3] * u2 + c[4] * v2 + c[5]  # (B, Ho, Wo) int64, GEOM_BITS fraction bits
    near, near_in = _nearest_index(X, Y, h, w, Wc)
    r5 = 1 << (GEOM_BITS - 6)
    X5, Y5 = (X + r5) >> (GEOM_BITS - 5), (Y + r5) >> (GEOM_BITS - 5)
    xi, yi, fx, fy = X5 >> 5, Y5 >> 5, X5 & 31, Y5 & 31
    q15, f32 = (t.to(dev) for t in cubic_table())

    def taps(src, r):  # the four taps of tap row r as (B, Ho, Wo, C) each, 0 outside the sample
        y = yi - 1 + r
        out = []
        for k in range(4):
            x = xi - 1 + k
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            idx = ((y.clamp(min=0) * Wc + x.clamp(min=0)) * inside).view(B, Ho * Wo, 1).expand(B, Ho * Wo, 3)
            val = src.view(B, Hc * Wc, 3).gather(1, idx).view(B, Ho, Wo, 3)
            out.append(torch.where(inside.unsqueeze(-1), val, torch.zeros_like(val)))
        return out

    def nearest(src):  # (B, Hc, Wc) -> (B, Ho, Wo)
        val = src.view(B, Hc * Wc).gather(1, near.view(B, Ho * Wo)).view(B, Ho, Wo)
        return torch.where(near_in, val, torch.zeros_like(val))

    # image: exact integer accumulation
    src = img.contiguous().to(torch.int64)
    wx, wy = q15.to(torch.int64)[fx], q15.to(torch.int64)[fy]  # (B, Ho, Wo, 4)
    acc = torch.zeros(B, Ho, Wo, 3, dtype=torch.int64, device=dev)
    for r in range(4):
        t = taps(src, r)
        hs = sum(wx[..., k:k + 1] * t[k] for k in range(4))
        acc = acc + wy[..., r:r + 1] * hs
    out = {"image": ((acc + (1 << 29)) >> 30).clamp(0, 255).to(torch.uint8).contiguous()}
    for t in tasks:
        k, src = task_kind(t), _as_tensor(raw[t]).to(dev).contiguous()
        if k in _U8_KINDS:
            out[t] = nearest(src).contiguous()
        elif k == "depth":
            out[t] = (nearest(src) / side[:, 2].view(B, 1, 1)).contiguous()
        else:  # normals: fp32, every product and sum rounded on its own, in this order
            fwx, fwy = f32[fx], f32[fy]
            n = None
            for r in range(4):
                tp = taps(src, r)
                hs = fwx[..., 0:1] * tp[0]
                for kk in range(1, 4):
                    hs = hs + fwx[..., kk:kk + 1] * tp[kk]
                m = fwy[..., r:r + 1] * hs
                n = m if n is None else n + m
            cs, sn = side[:, 0].view(B, 1, 1), side[:, 1].view(B, 1, 1)
            x, y, z = n[..., 0] * cs + n[..., 1] * sn, n[..., 1] * cs - n[..., 0] * sn, n[..., 2]
            if renormalize:
                # the correctly rounded fp32 square root, through float64 (53 >= 2 * 24 + 2 bits: rounding twice is rounding once);
                # torch's own fp32 sqrt on a CPU is a vector-library routine that can be one unit in the last place off
                root = torch.sqrt(((x * x + y * y) + z * z).to(torch.float64)).to(torch.float32)
                d = root + torch.tensor(NORMALS_EPS, dtype=torch.float32, device=dev)
                x, y, z = x / d, y / d, z / d
            out[t] = torch.stack([x, y, z], dim=-1).contiguous()
    if raw.get("flip") is not None:
        out["flip"] = _as_tensor(raw["flip"])
    return out


_cubic_dev: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}


def augment_batch(raw: Mapping, tasks: Sequence[str], geom: Geometry, out_size, renormalize: bool = True):
    """``augment_batch_torch`` of a raw batch that already lives on the GPU, as ONE library call and one launch on the current
    stream (csrc/augment.hip, no host sync).  ``geom`` may live on the host (it is copied) or on the device.  Returns the
    wire-format batch ``prepare_batch`` takes; GPU only, there is no CPU fallback."""
    from . import functional as Fn
    B, Hc, Wc = check_raw_batch(raw, tasks)
    Ho, Wo = _out_size(out_size)
    img = raw["image"]
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise RuntimeError("mtlora_amd: augment_batch takes a batch on a ROCm GPU (MI355X); the HIP path has no CPU fallback "
                           "(data.augment_batch_torch is the portable restatement)")
    if len(tasks) + 1 > L.INGEST_MAX_JOBS:
        raise RuntimeError(f"mtlora_amd: augment_batch takes at most {L.INGEST_MAX_JOBS - 1} tasks per call")
    dev = img.device
    key = str(dev)
    if key not in _cubic_dev:
        _cubic_dev[key] = tuple(t.to(dev) for t in cubic_table())
    q15, f32 = _cubic_dev[key]
    jobs = [("image_cubic_u8", img)] + [(_AUG_KIND[task_kind(t)], raw[t]) for t in tasks]
    outs = Fn.augment_batch(jobs, _as_tensor(raw["size"]).to(dev), _as_tensor(geom.coef).to(dev), _as_tensor(geom.side).to(dev),
                            (Ho, Wo), cubic_q15=q15, cubic_f32=f32, renormalize=renormalize)
    out = dict(zip(["image"] + list(tasks), outs))
    if raw.get("flip") is not None:
        out["flip"] = raw["flip"]
    return out


def synthetic_raw_batch(B: int, Hc: int, Wc: int, tasks: Sequence[str], seed: int, sizes=None,
                        num_outputs: Optional[Mapping[str, int]] = None) -> Dict[str, torch.Tensor]:
    """a host batch in canvas format with the label distributions of ``synthetic_wire_batch`` inside each sample's rectangle and
    a non-zero sentinel outside it (image 165, class maps 200, normals 7.0, depth 99.0: a value that leaks into an output shows).
    ``sizes``: (B, 2) integers (h, w); default: drawn from the seed in [Hc / 2, Hc] x [Wc / 2, Wc]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if sizes is None:
        size = torch.stack([torch.randint((Hc + 1) // 2, Hc + 1, (B,), generator=g), torch.randint((Wc + 1) // 2, Wc + 1, (B,), generator=g)], 1)
    else:
        size = torch.as_tensor(sizes).reshape(B, 2)
    size = size.to(torch.int32).contiguous()
    out = {"image": torch.randint(0, 256, (B, Hc, Wc, 3), generator=g, dtype=torch.uint8)}
    sentinel = {"image": 165}
    for t in tasks:
        k = task_kind(t)
        if k in ("semseg", "human_parts"):
            lab = torch.randint(0, int((num_outputs or {}).get(t, NUM_OUTPUT[k])), (B, Hc, Wc), generator=g, dtype=torch.uint8)
            lab[torch.rand(B, Hc, Wc, generator=g) < 0.05] = 255
        elif k == "sal":
            lab = (torch.rand(B, Hc, Wc, generator=g) < 0.3).to(torch.uint8)
        elif k == "normals":
            lab = torch.nn.functional.normalize(torch.randn(B, Hc, Wc, 3, generator=g), dim=-1)
            lab[torch.rand(B, Hc, Wc, generator=g) < 0.05] = 0.0
        elif k == "depth":
            lab = torch.rand(B, Hc, Wc, generator=g) * 10
        elif k == "edge":
            lab = (torch.rand(B, Hc, Wc, generator=g) < 0.1).to(torch.uint8)
        else:
            raise NotImplementedError(t)
        out[t] = lab.contiguous()
        sentinel[t] = 200 if k in _U8_KINDS else (7.0 if k == "normals" else 99.0)
    rows, cols = torch.arange(Hc).view(1, Hc, 1), torch.arange(Wc).view(1, 1, Wc)
    outside = (rows >= size[:, 0].view(B, 1, 1)) | (cols >= size[:, 1].view(B, 1, 1))
    for k, v in out.items():
        v[outside] = sentinel[k]
    out["size"] = size
    return out


class DeviceLoader:
    """Wraps any iterable of wire-format host batches and yields ``(images, targets)`` on ``device``, ready for
    ``train_step``, ``validate_step`` and ``predict``.  A host batch that carries ``valid`` (a partially labelled batch, see the
    module docstring) yields ``(images, targets, valid)``: the flags travel through the ring with the tensors and arrive as
    fresh uint8 tensors on ``device``, what ``train_step(valid=)`` takes.

    A ring of ``depth`` pinned staging sets (host and device side) is filled ahead of the consumer: the host-to-device
    copies and ``prepare_batch`` of the next batches run on a side stream while the consumer works on the current one; an
    event makes the consumer's current stream wait for exactly the batch it receives.  The yielded tensors are fresh
    allocations, never part of the ring, and are marked (``record_stream``) as used on the consumer's stream, so they stay
    valid for as long as the consumer holds them.  A staging set is reused only after the ``prepare_batch`` that read it has
    finished (its event is waited for on the host before the pinned buffers are overwritten).  A host tensor that is
    already pinned (a ``DataLoader`` with ``pin_memory=True``) is copied from where it is and kept alive until then.

    ``flip_p``: probability of the horizontal flip per sample; the flags come from a host ``torch.Generator`` seeded with
    ``seed`` (one draw of B numbers per batch, in order), so a seed reproduces an epoch.  A ``flip`` entry in a host batch
    takes precedence.  GPU only.

    ``out_size=(Ho, Wo)``: the iterable yields RAW canvas-format batches (``check_raw_batch``) instead, and ``augment_batch``
    runs in front of ``prepare_batch`` on the side stream; ``size`` and the geometry travel through the pinned ring with the
    tensors.  With ``augment=None`` that is resize-only (rotation 0, scale 1: the reference's test pipeline, mtl_ds.py:866-867)
    and draws nothing.  ``augment=dict(rots=(-20, 20), scales=(.75, 1.25))`` is ``ScaleNRotate``'s continuous form
    (custom_transforms.py:42-48: ``rot = (hi - lo) r - (hi - lo) / 2``, ``sc = (hi - lo) r - (hi - lo) / 2 + 1`` with r uniform
    in [0, 1)), ``augment=dict(rots=[0], scales=[1.0, 1.2, 1.5])`` the list form (:49-52, a uniform pick of each).  Per batch
    the flips are drawn first, exactly as without ``augment``, then B numbers for ``rot`` and B for ``scale`` from the same
    generator; ``rot_deg`` and ``scale`` entries in a host batch take precedence, as ``flip`` does.  ``last_geoms`` holds the
    ``Geometry`` of every batch of the epoch next to ``last_flips``."""

    def __init__(self, batches: Iterable[Mapping], tasks: Sequence[str], device, flip_p: float = 0.0, seed: int = 0,
                 depth: int = 2, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 augment: Optional[Mapping] = None, out_size=None):
        if not 0.0 <= float(flip_p) <= 1.0:
            raise ValueError(f"DeviceLoader: flip_p must be in [0, 1], got {flip_p}")
        if int(depth) != depth or depth < 1:
            raise ValueError(f"DeviceLoader: depth must be an integer >= 1, got {depth}")
        if len(tasks) == 0 or len(tasks) + 1 > L.INGEST_MAX_JOBS:
            raise ValueError(f"DeviceLoader: 1 to {L.INGEST_MAX_JOBS - 1} tasks, got {len(tasks)}")
        for t in tasks:
            if task_kind(t) not in _JOB_KIND:
                raise ValueError(f"DeviceLoader: unknown task {t!r}")
        if augment is not None:
            if out_size is None:
                raise ValueError("DeviceLoader: augment needs out_size")
            if not isinstance(augment, Mapping) or set(augment) != {"rots", "scales"}:
                raise ValueError(f"DeviceLoader: augment must be dict(rots=..., scales=...), got {augment!r}")
            rots, scales = augment["rots"], augment["scales"]
            if type(rots) is not type(scales) or not isinstance(rots, (tuple, list)):  # (custom_transforms.py:35)
                raise ValueError("DeviceLoader: augment rots and scales must be two (lo, hi) tuples or two lists")
            try:
                rots, scales = type(rots)(float(v) for v in rots), type(scales)(float(v) for v in scales)
            except (TypeError, ValueError):
                raise ValueError(f"DeviceLoader: augment rots and scales must hold numbers, got {augment!r}") from None
            if not all(math.isfinite(v) for v in list(rots) + list(scales)):
                raise ValueError(f"DeviceLoader: augment rots and scales must be finite, got {augment!r}")
            if isinstance(rots, tuple):
                if len(rots) != 2 or len(scales) != 2 or rots[0] > rots[1] or scales[0] > scales[1]:
                    raise ValueError(f"DeviceLoader: the continuous form takes (lo, hi) with lo <= hi, got {augment!r}")
                if 1.0 - (scales[1] - scales[0]) / 2 <= 0.0:
                    raise ValueError(f"DeviceLoader: scales {scales} can draw a scale <= 0")
            elif len(rots) == 0 or len(scales) == 0 or min(scales) <= 0.0:
                raise ValueError(f"DeviceLoader: the list form takes non-empty lists and scales > 0, got {augment!r}")
            augment = {"rots": rots, "scales": scales}
        if out_size is not None:
            try:
                out_size = _out_size(out_size)
            except ValueError as e:
                raise ValueError(f"DeviceLoader: {e}") from None
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mtlora_amd: DeviceLoader needs a ROCm GPU (MI355X) device; the HIP path has no CPU fallback")
        self.augment, self.out_size = augment, out_size
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

    def _draw_geometry(self, host: Mapping, B: int, gen: torch.Generator) -> Geometry:
        """rot and scale of the B samples (host entries first, else the draws: rot, then scale) and their ``make_geometry``"""
        def given(key):
            v = host.get(key)
            if v is None:
                return None
            v = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
            if v.shape[0] != B:
                raise ValueError(f"raw batch: {key} must hold {B} numbers, got {tuple(v.shape)}")
            return v

        rot, sc = given("rot_deg"), given("scale")
        if self.augment is None:
            rot = torch.zeros(B, dtype=torch.float64) if rot is None else rot
            sc = torch.ones(B, dtype=torch.float64) if sc is None else sc
        else:
            rots, scales = self.augment["rots"], self.augment["scales"]
            for which, vals in (("rot", rots), ("sc", scales)):
                if (rot if which == "rot" else sc) is not None:
                    continue
                if isinstance(vals, tuple):
                    span = vals[1] - vals[0]
                    v = span * torch.rand(B, generator=gen, dtype=torch.float64) - span / 2 + (0.0 if which == "rot" else 1.0)
                else:
                    v = torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (B,), generator=gen)]
                if which == "rot":
                    rot = v
                else:
                    sc = v
        return make_geometry(_as_tensor(host["size"]), rot, sc, self.out_size)

    def _submit(self, slot: int, host: Mapping, gen: torch.Generator):
        keys = ["image"] + self.tasks
        raw = self.out_size is not None
        B = (check_raw_batch if raw else check_wire_batch)(host, self.tasks)[0]
        if raw:
            _check_valid(host, self.tasks, B, "raw batch")
        if host.get("flip") is not None:
            flip = _as_tensor(host["flip"])
        elif self.flip_p > 0.0:
            flip = (torch.rand(B, generator=gen) < self.flip_p).to(torch.uint8)
        else:
            flip = None
        geom = self._draw_geometry(host, B, gen) if raw else None
        extra = {"flip": flip} if flip is not None else {}
        extra.update({"valid:" + t: _as_tensor(v) for t, v in (host.get("valid") or {}).items()})
        if raw:
            extra.update(size=_as_tensor(host["size"]), coef=geom.coef, side=geom.side)
        entry = self._ring[slot]
        if entry["done"] is not None:
            entry["done"].synchronize()  # the ingest that read this slot's device buffers (and so its copies) has finished
        entry["hold"] = []
        dev_batch = {}
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            for k in keys + list(extra):
                src = extra[k] if k in extra else _as_tensor(host[k])
                direct = src.is_pinned() and src.is_contiguous()  # (a DataLoader with pin_memory=True: copied from where it is)
                pinned, on_dev = self._staging(slot, k, src, pinned=not direct)
                if direct:
                    entry["hold"].append(src)  # alive until this slot's event has passed
                else:
                    pinned.copy_(src)
                on_dev.copy_(src if direct else pinned, non_blocking=True)
                dev_batch[k] = on_dev
            # (the yielded flags are copies: the ring's buffers are overwritten by a later batch)
            valid = {k[6:]: dev_batch.pop(k).clone() for k in list(dev_batch) if k.startswith("valid:")}
            if raw:  # the wire-format intermediate is an allocation of the side stream, consumed on it right away
                dev_batch = augment_batch(dev_batch, self.tasks, Geometry(dev_batch.pop("coef"), dev_batch.pop("side")), self.out_size)
            out = prepare_batch(dev_batch, self.tasks, mean=self.mean, std=self.std)
            if valid:
                out = (out[0], out[1], valid)
            entry["done"] = torch.cuda.Event()
            entry["done"].record(self._stream)
        return out, entry["done"], flip, geom

    def __iter__(self):
        with torch.cuda.device(self.device):
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=self.device)
        self._ring = [{"buf": {}, "done": None, "hold": []} for _ in range(self.depth)]
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self.last_flips, self.last_geoms = [], []
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
            out, done, flip, geom = pending.pop(0)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(done)
            for t in [out[0]] + [x for d in out[1:] for x in d.values()]:
                t.record_stream(cur)
            self.last_flips.append(flip)
            self.last_geoms.append(geom)
            yield out
