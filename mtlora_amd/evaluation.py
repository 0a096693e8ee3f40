"""Validation metrics of the six tasks: the API of the reference's ``evaluation.evaluate_utils`` (``get_output``,
``PerformanceMeter``, ``calculate_multi_task_performance``), restated so that a reference user changes one import:

    from mtlora_amd.evaluation import PerformanceMeter, get_output, calculate_multi_task_performance

Two ways in:

* ``PerformanceMeter.update(pred, gt)`` takes processed full-resolution predictions (``get_output`` of the model's output) like
  the reference.  Plain torch, works on CPU and GPU.
* ``PerformanceMeter.update_low(low, gt)`` takes the LOW-resolution (B, h, w, C) head outputs of ``model(x, upsample=False)``: the
  final bilinear upsample, ``get_output``, the meter update and the task's loss are ONE launch per task (csrc/metrics.hip); the
  full-resolution prediction never exists.

Meter state is tensors (int64 counts, fp64 sums) on the device of the data; neither ``update`` nor ``update_low`` synchronises
with the host, ``get_score()`` does the only device-to-host copy.  ``get_score`` returns the reference's dict keys.

Differences from the reference, on purpose: counts are int64 (SaliencyMeterWithBeta accumulates fp32, exact only up to 2^24
pixels); ``reset()`` resets every meter (DepthMeter.reset leaves its totals, eval_depth.py:91-93); a batch of one image works
(``squeeze()`` drops the batch axis in eval_sal_no_beta.py:36-37).  Kept from the reference, on purpose: both normals meters report
``rmse == mean`` (eval_normals_v1.py:63, eval_normals_v2.py:49); the with-beta saliency meter applies a second sigmoid to the
probability (eval_sal_beta.py:37-52); the edge meter evaluates the loss on the PROCESSED prediction (eval_edge.py:31-34).

Reference: evaluation/evaluate_utils.py:20-126, eval_semseg.py:88-148, eval_human_parts.py:86-131, eval_normals*.py,
eval_sal*.py + jaccard.py, eval_depth.py:65-108, eval_edge.py:23-50.
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

EDGE_POS_WEIGHT = 0.95  # evaluate_utils.py:122
SEMSEG_CLASSES = {"PASCALContext": 21, "NYUD": 40}  # eval_semseg.py:90-103 (20 + background, 40)
FUSED_KIND = {"semseg": "softmax", "human_parts": "softmax", "normals": "normals", "sal": "saliency", "depth": "l1_masked",
              "edge": "edge"}


def get_output(output: torch.Tensor, task: str) -> torch.Tensor:
    """(B, C, H, W) model output -> what the meters take, channels last (evaluate_utils.py:20-38): unit normals mapped to
    [0, 255], class ids, 255 * sigmoid, or the depth itself."""
    output = output.permute(0, 2, 3, 1)
    if task == "normals":
        return (F.normalize(output, p=2, dim=3) + 1.0) * 255 / 2.0
    if task in ("semseg", "human_parts"):
        return torch.max(output, dim=3)[1]
    if task in ("edge", "sal"):
        return torch.squeeze(255 * 1 / (1 + torch.exp(-output)))
    if task == "depth":
        return output
    raise ValueError("Select one of the valid tasks")


PREDICT_KIND = {"semseg": "argmax", "human_parts": "argmax", "normals": "normals", "sal": "sigmoid", "edge": "sigmoid",
                "depth": "identity"}


def get_output_low(low: torch.Tensor, task: str, scale: int, uint8: bool = False) -> torch.Tensor:
    """the fused twin of ``get_output``: ``get_output(F.interpolate(low.permute(0, 3, 1, 2), scale_factor=scale,
    mode="bilinear"), task)`` from the LOW-resolution (B, h, w, C) head output of ``model(x, upsample=False)`` in one launch
    (csrc/predict.hip); the full-resolution logits never exist.  GPU only.  Shapes are ``get_output``'s for B > 1 -- the batch
    axis of one image is kept, where the reference's ``squeeze()`` drops it -- and class maps are uint8 (``PerformanceMeter.update``
    takes them).  ``uint8=True``: the [0, 255] images of normals / sal / edge truncated to uint8, ready to be written out."""
    from . import functional as Fn
    if task not in PREDICT_KIND:
        raise ValueError("Select one of the valid tasks")
    kind = PREDICT_KIND[task]
    return Fn.upsample_predict(kind, low, scale, out_dtype=torch.uint8 if (uint8 and kind in ("normals", "sigmoid")) else None)


class _Meter:
    """state: ``counts`` (int64) and ``sums`` (fp64) tensors, created on the device of the first batch"""
    n_counts, n_sums = 0, 0

    def __init__(self):
        self.reset()

    def reset(self):
        self.counts: Optional[torch.Tensor] = None
        self.sums: Optional[torch.Tensor] = None

    def _state(self, device):
        if self.counts is None:
            self.counts = torch.zeros(max(self.n_counts, 1), dtype=torch.int64, device=device)
            self.sums = torch.zeros(max(self.n_sums, 1), dtype=torch.float64, device=device)
        elif self.counts.device != device:
            self.counts, self.sums = self.counts.to(device), self.sums.to(device)

    @staticmethod
    def _labelled(pred, gt, valid):
        """the portable definition of ``update(pred, gt, valid)``: the labelled samples index-selected (``valid`` (B,), non-zero:
        the sample carries a label for this task; read on the host, as ``functional.upsample_loss_valid_torch`` does).  Returns
        ``(pred, gt)`` as they are when every sample is labelled, the sub-batch otherwise, ``None`` when there is none."""
        B = gt.shape[0]
        flags = torch.as_tensor(valid).reshape(-1)
        if flags.numel() != B:
            raise RuntimeError(f"mtlora_amd: valid must have one flag per sample ({B}), got {flags.numel()}")
        idx = torch.nonzero(flags != 0).reshape(-1)
        if idx.numel() == B:
            return pred, gt
        if idx.numel() == 0:
            return None
        return pred.index_select(0, idx.to(pred.device)), gt.index_select(0, idx.to(gt.device))

    def _host(self):
        if self.counts is None:
            raise RuntimeError("mtlora_amd: get_score() of a meter that has seen no batch")
        return self.counts.cpu().tolist(), self.sums.cpu().tolist()


class SegmentationMeter(_Meter):
    """SemsegMeter / HumanPartsMeter: per-class tp / fp / fn among label != 255.  counts: tp[C], predicted[C], gt[C], valid."""

    def __init__(self, n_classes: int, name: str = "Semantic Segmentation"):
        self.n_classes, self.name = int(n_classes), name
        self.n_counts = 3 * self.n_classes + 1
        super().__init__()

    @torch.no_grad()
    def update(self, pred, gt, valid=None):
        if valid is not None:
            sel = self._labelled(pred, gt, valid)
            if sel is None:
                return
            pred, gt = sel
        C = self.n_classes
        self._state(gt.device)
        g = gt.reshape(-1)
        p = pred.reshape(-1).to(g.dtype)
        valid = g != 255
        gi, pi = g.clamp(0, C - 1).long(), p.clamp(0, C - 1).long()
        g_in, p_in = valid & (g >= 0) & (g < C) & (g == gi), valid & (p >= 0) & (p < C)
        self.counts.index_add_(0, gi, (g_in & (p == g)).long())
        self.counts.index_add_(0, pi + C, p_in.long())
        self.counts.index_add_(0, gi + 2 * C, g_in.long())
        self.counts[3 * C] += valid.sum()

    def update_fused(self, low, gt, scale, valid=None):
        from . import functional as Fn
        if low.shape[-1] != self.n_classes:
            raise RuntimeError(f"mtlora_amd: {self.name} meter has {self.n_classes} classes, the prediction {low.shape[-1]}")
        self._state(low.device)
        _, sums = Fn.upsample_metrics("softmax", low, gt, scale, counts=self.counts, valid=valid)
        return sums[0]

    def get_score(self, verbose=True):
        c, _ = self._host()
        C = self.n_classes
        jac = [float(c[i]) / max(float(c[C + i] + c[2 * C + i] - c[i]), 1e-8) for i in range(C)]  # tp / (tp + fp + fn)
        res = {"jaccards_all_categs": jac, "mIoU": np.mean(jac)}
        if verbose:
            print("\n{0:s} mIoU: {1:.4f}\n".format(self.name, 100 * res["mIoU"]))
            for i, j in enumerate(jac):
                print("class {0:<10d}{1:.4f}".format(i, 100 * j))
        return res


class NormalsMeter(_Meter):
    """NormalsMeterV1 + NormalsMeterV2.  counts: n_v1, #<11.25, #<22.5, #<30, n_v2; sums: V1 degrees, V2 degrees."""
    n_counts, n_sums = 5, 2

    @staticmethod
    def _unit(x):
        n = torch.norm(x, p="fro", dim=1, keepdim=True)
        zero = n == 0
        return torch.where(zero.expand_as(x), torch.zeros_like(x), x / torch.where(zero, torch.ones_like(n), n))

    @torch.no_grad()
    def update(self, pred, gt, valid=None):
        if valid is not None:
            sel = self._labelled(pred, gt, valid)
            if sel is None:
                return
            pred, gt = sel
        self._state(gt.device)
        p = (2 * pred / 255 - 1).permute(0, 3, 1, 2)
        ok = gt != 255
        zero = torch.zeros_like(p)
        d1 = (180 / math.pi) * torch.acos(torch.clamp(torch.sum(torch.where(ok, p, zero) * torch.where(ok, gt, zero), 1), min=-1, max=1))
        m1 = ok[:, 0]
        pn, gn = self._unit(p), self._unit(gt)
        d2 = torch.rad2deg(2 * torch.atan2(torch.norm(pn - gn, dim=1), torch.norm(pn + gn, dim=1)))
        m2 = ok.all(dim=1)
        z = torch.zeros_like(d1)
        self.counts += torch.stack([m1.sum(), (m1 & (d1 < 11.25)).sum(), (m1 & (d1 < 22.5)).sum(), (m1 & (d1 < 30)).sum(), m2.sum()])
        self.sums += torch.stack([torch.where(m1, d1, z).sum(dtype=torch.float64), torch.where(m2, d2, z).sum(dtype=torch.float64)])

    def update_fused(self, low, gt, scale, valid=None):
        from . import functional as Fn
        self._state(low.device)
        _, sums = Fn.upsample_metrics("normals", low, gt, scale, counts=self.counts, valid=valid)
        self.sums += sums[1:3]
        return sums[0]

    def get_score(self, verbose=True):
        c, s = self._host()
        mean1, mean2 = s[0] / c[0], s[1] / c[4]
        res = {"mean": mean1, "rmse": mean1, "mean_v2": mean2, "rmse_v2": mean2}  # (rmse == mean: the reference's, see above)
        self.bins = {"11.25": 100.0 * c[1] / c[0], "22.5": 100.0 * c[2] / c[0], "30": 100.0 * c[3] / c[0]}
        if verbose:
            print("\nResults for Surface Normal Estimation")
            for k, v in res.items():
                print("{0:s}: {1:.4f}".format(k, v))
        return res


class SaliencyMeter(_Meter):
    """SaliencyMeterWithBeta (global counts over 19 thresholds) + SaliencyMeterWithNoBeta (per-image tp / fp / fn over 15).
    counts: [19][tp, predicted, actual]; ``per_image``: one (B, 15, 3) int64 tensor per batch; ``per_image_valid``: per batch,
    ``None`` (every row counts) or a device copy of the (B,) flags ``update_fused(valid=)`` was given -- the fused launch leaves
    an unlabelled image's row at zero, and ``get_score()`` drops it (an all-zero row would score a Jaccard of 1)."""
    n_counts = 57

    def __init__(self, beta_squared: float = 0.3):
        self.beta_squared = beta_squared
        self.mask_thres = np.linspace(0.2, 0.9, 15)
        self.thresholds = torch.arange(0.05, 1, 0.05)
        super().__init__()

    def reset(self):
        super().reset()
        self.per_image = []
        self.per_image_valid = []

    @torch.no_grad()
    def update(self, pred, gt, valid=None):
        if valid is not None:
            sel = self._labelled(pred, gt, valid)
            if sel is None:
                return
            pred, gt = sel
        self._state(gt.device)
        B = gt.shape[0]
        p = pred.float().reshape(B, -1) / 255.
        g = gt.reshape(B, -1)
        gpos = g != 0
        rows = []
        for t in self.mask_thres:
            m = p > t
            tp = (m & gpos).sum(1)
            rows.append(torch.stack([tp, m.sum(1) - tp, gpos.sum(1) - tp], 1))
        self.per_image.append(torch.stack(rows, 1))
        self.per_image_valid.append(None)
        q = torch.sigmoid(p)
        valid = g != 255
        tg = torch.where(valid, g.long(), torch.zeros_like(g, dtype=torch.long))
        ap = tg.sum()
        cols = []
        for t in self.thresholds.to(q.device):
            f = ((q >= t) & valid).long()
            cols.append(torch.stack([(f * tg).sum(), f.sum(), ap]))
        self.counts += torch.stack(cols).reshape(-1)

    def update_fused(self, low, gt, scale, valid=None):
        from . import functional as Fn
        self._state(low.device)
        B = low.shape[0]
        counts, sums = Fn.upsample_metrics("saliency", low, gt, scale, valid=valid)
        self.counts += counts[:57]
        self.per_image.append(counts[57:57 + 45 * B].view(B, 15, 3))
        self.per_image_valid.append(None if valid is None else valid.clone())  # (the caller may rewrite its buffer)
        return sums[0]

    def _per_image_rows(self):
        """(N, 15, 3) on the host: the rows of the labelled images of every batch"""
        im = torch.cat(self.per_image).cpu()
        if any(v is not None for v in self.per_image_valid):
            keep = torch.cat([torch.ones(r.shape[0], dtype=torch.bool) if v is None else v.cpu() != 0
                              for r, v in zip(self.per_image, self.per_image_valid)])
            im = im[keep]
        return im.numpy()

    def get_score(self, verbose=True):
        c, _ = self._host()
        g = torch.tensor(c, dtype=torch.int64).view(19, 3)
        tp, pp, ap = g[:, 0].float(), g[:, 1].float(), g[:, 2].float()
        precision, recall = tp / pp, tp / ap
        fscore = (1 + self.beta_squared) * precision * recall / (self.beta_squared * precision + recall)
        fscore[fscore != fscore] = 0
        im = self._per_image_rows()  # (N, 15, 3)
        tp, fp, fn = im[..., 0], im[..., 1], im[..., 2]
        union = (tp + fp + fn).astype(float)
        jac = np.where(union == 0, 1.0, tp / np.where(union == 0, 1.0, union))  # jaccard.py:27-28: nothing there, nothing found
        m_prec, m_rec = np.mean(tp / (tp + fp + 1e-12), 0), np.mean(tp / (tp + fn + 1e-12), 0)
        f = 2 * m_prec * m_rec / (m_prec + m_rec + 1e-12)
        res = {"Beta maxF": fscore.max().item(), "maxF": float(np.max(f)), "mIoU": float(np.max(np.mean(jac, 0)))}
        if verbose:
            print("\nResults for Saliency Estimation")
            for k, v in res.items():
                print("{0:s}: {1:.3f}".format(k, 100.0 * v))
        return res


class DepthMeter(_Meter):
    """counts: valid; sums: (gt - p)^2, (log gt - log p)^2 with p = max(pred, 1e-9), over label != 255."""
    n_counts, n_sums = 1, 2

    @torch.no_grad()
    def update(self, pred, gt, valid=None):
        if valid is not None:
            sel = self._labelled(pred, gt, valid)
            if sel is None:
                return
            pred, gt = sel
        self._state(gt.device)
        g = gt.reshape(-1)
        p = torch.clamp(pred.reshape(-1), min=1e-9)
        mask = g != 255
        z = torch.zeros_like(p)
        self.counts += mask.sum()
        self.sums += torch.stack([torch.where(mask, torch.pow(g - p, 2), z).sum(dtype=torch.float64),
                                  torch.where(mask, torch.pow(torch.log(g) - torch.log(p), 2), z).sum(dtype=torch.float64)])

    def update_fused(self, low, gt, scale, valid=None):
        from . import functional as Fn
        self._state(low.device)
        _, sums = Fn.upsample_metrics("l1_masked", low, gt, scale, counts=self.counts, valid=valid)
        self.sums += sums[1:3]
        return sums[0]

    def get_score(self, verbose=True):
        c, s = self._host()
        res = {"rmse": np.sqrt(s[0] / c[0]), "log_rmse": np.sqrt(s[1] / c[0])}
        if verbose:
            print("Results for depth prediction")
            for k, v in res.items():
                print("{0:<15s}{1:.4f}".format(k, v))
        return res


class EdgeMeter(_Meter):
    """the edge loss on the processed prediction, weighted by the batch's element count (the true edge score, seism's odsF, is
    computed offline in the reference as well).  sums: numel * loss; ``n``: elements seen (a host integer); ``n_dev``: the
    elements of the batches ``update_fused(valid=)`` saw, |V| H W each, counted on the device and read in ``get_score()``."""
    n_sums = 1

    def __init__(self, pos_weight: float = EDGE_POS_WEIGHT):
        self.pos_weight = pos_weight
        super().__init__()

    def reset(self):
        super().reset()
        self.n = 0
        self.n_dev: Optional[torch.Tensor] = None

    @torch.no_grad()
    def update(self, pred, gt, valid=None):
        if valid is not None:
            sel = self._labelled(pred, gt, valid)
            if sel is None:
                return
            pred, gt = sel
        self._state(gt.device)
        g = gt.reshape(-1).float()
        o = pred.float().reshape(-1) / 255.
        labels = (g >= 0.5).float()
        gz = (o >= 0).float()
        lv = o * (labels - gz) - torch.log(1 + torch.exp(o - 2 * o * gz))
        w = self.pos_weight
        loss = (w * (-(labels * lv)).sum() + (1 - w) * (-((1.0 - labels) * lv)).sum()) / float(g.numel())
        self.n += g.numel()
        self.sums += loss.double() * g.numel()

    def update_fused(self, low, gt, scale, valid=None):
        from . import functional as Fn
        self._state(low.device)
        _, sums = Fn.upsample_metrics("edge", low, gt, scale, pos_weight=self.pos_weight, valid=valid)
        if valid is None:
            self.n += gt.numel()
            self.sums += sums[1:2] * gt.numel()
        else:  # the launch normalised by |V| H W
            n = (valid != 0).sum() * (gt.numel() // max(gt.shape[0], 1))
            self.n_dev = n if self.n_dev is None else self.n_dev + n
            self.sums += sums[1:2] * n
        return sums[0]

    def get_score(self, verbose=True):
        _, s = self._host()
        n = self.n + (0 if self.n_dev is None else int(self.n_dev.item()))
        res = {"loss": s[0] / n if n else float("nan")}  # (only batches without a labelled sample: no score)
        if verbose:
            print("\nEdge Detection Evaluation")
            print("Edge Detection Loss %.3f" % res["loss"])
        return res


def get_single_task_meter(task: str, database: str = "PASCALContext", num_outputs: Optional[Mapping[str, int]] = None):
    """the meter of one task (evaluate_utils.py:96-126)"""
    if task == "semseg":
        if database not in SEMSEG_CLASSES and not (num_outputs and "semseg" in num_outputs):
            raise NotImplementedError(database)
        return SegmentationMeter((num_outputs or {}).get("semseg", SEMSEG_CLASSES.get(database)), "Semantic Segmentation")
    if task == "human_parts":
        return SegmentationMeter((num_outputs or {}).get("human_parts", 7), "Human Parts")
    if task == "normals":
        return NormalsMeter()
    if task == "sal":
        return SaliencyMeter()
    if task == "depth":
        return DepthMeter()
    if task == "edge":
        return EdgeMeter(pos_weight=EDGE_POS_WEIGHT)
    raise NotImplementedError(task)


class PerformanceMeter:
    """a meter per task (evaluate_utils.py:41-63).  ``tasks``: the task names, or the reference's config object (``.TASKS``)."""

    def __init__(self, tasks, database: str = "PASCALContext", num_outputs: Optional[Mapping[str, int]] = None):
        self.database = database
        self.tasks = list(getattr(tasks, "TASKS", tasks))
        self.meters = {t: get_single_task_meter(t, database, num_outputs) for t in self.tasks}

    def reset(self):
        for t in self.tasks:
            self.meters[t].reset()

    def update(self, pred: Mapping[str, torch.Tensor], gt: Mapping[str, torch.Tensor],
               valid: Optional[Mapping[str, torch.Tensor]] = None):
        """``valid`` (partially labelled batches): ``{task: uint8 (B,)}``, non-zero: the sample carries a label for the task; a
        task without an entry is labelled everywhere.  A task's meter then sees its labelled samples only."""
        for t in self.tasks:
            v = None if valid is None else valid.get(t)
            if v is None:
                self.meters[t].update(pred[t], gt[t])
            else:
                self.meters[t].update(pred[t], gt[t], v)

    def update_task_low(self, t: str, lo: torch.Tensor, lab: torch.Tensor, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one task's meter from its LOW-resolution (B, h, w, C) prediction; returns the task's loss (a device scalar).  Fused
        under the conditions of ``MultiTaskLoss.task_low`` (GPU, integer scale), else ``update(get_output(interpolate))``.
        ``valid``: this task's uint8 (B,) flags; meter and loss then cover the labelled samples only (fused: the flags are read
        on the device, nothing comes back to the host)."""
        h, w = lo.shape[1:3]
        H, W = lab.shape[-2:]
        if lo.is_cuda and H % h == 0 and W % w == 0 and H // h == W // w:
            if valid is None:
                return self.meters[t].update_fused(lo, lab, H // h)
            return self.meters[t].update_fused(lo, lab, H // h, valid)
        from .mtl_harness import task_loss
        up = F.interpolate(lo.permute(0, 3, 1, 2).float(), (H, W), mode="bilinear")
        if valid is None:
            self.meters[t].update(get_output(up, t), lab)
            return task_loss(t, up, lab)
        self.meters[t].update(get_output(up, t), lab, valid)
        return task_loss(t, up, lab, valid=valid)

    def update_low(self, low: Mapping[str, torch.Tensor], gt: Mapping[str, torch.Tensor],
                   valid: Optional[Mapping[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """the fused path: ``low`` is the dict of (B, h, w, C) head outputs of ``model(x, upsample=False)``.  One launch per
        task, no host sync; returns the per-task losses.  ``valid``: ``{task: uint8 (B,)}`` as ``update``."""
        return {t: self.update_task_low(t, low[t], gt[t], None if valid is None else valid.get(t)) for t in self.tasks}

    def get_score(self, verbose: bool = True):
        return {t: self.meters[t].get_score(verbose) for t in self.tasks}


def calculate_multi_task_performance(eval_dict, single_task_dict):
    """mean relative improvement over the single-task scores, signs so that larger is better (evaluate_utils.py:66-91)"""
    assert set(eval_dict.keys()) == set(single_task_dict.keys())
    perf = 0.0
    for task in eval_dict:
        mtl, stl = eval_dict[task], single_task_dict[task]
        if task == "depth":
            perf -= (mtl["rmse"] - stl["rmse"]) / stl["rmse"]
        elif task in ("semseg", "sal", "human_parts"):
            perf += (mtl["mIoU"] - stl["mIoU"]) / stl["mIoU"]
        elif task == "normals":
            perf -= (mtl["mean"] - stl["mean"]) / stl["mean"]
        elif task == "edge":
            perf += (mtl["odsF"] - stl["odsF"]) / stl["odsF"]
        else:
            raise NotImplementedError
    return perf / len(eval_dict)
