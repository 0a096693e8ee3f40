"""Partially labelled batches at the measuring end, on the CPU: every meter's ``update(pred, gt, valid)`` is the portable
definition -- index-select the labelled samples, then today's update -- and ``PerformanceMeter.update(valid=)`` hands a
``{task: uint8 (B,)}`` dict through.  All six tasks, B = 4, 16 x 16 labels; meter states are compared exactly (the same torch
ops on the same sub-batch)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mtlora_amd.evaluation import PerformanceMeter, get_output, get_single_task_meter

ALL6 = ["semseg", "human_parts", "normals", "sal", "depth", "edge"]
CH = {"semseg": 21, "human_parts": 7, "normals": 3, "sal": 1, "depth": 1, "edge": 1}
B, S = 4, 16
MASKS = {"first": [1, 0, 0, 0], "last": [0, 0, 0, 1], "alternating": [1, 0, 1, 0], "all": [1, 1, 1, 1]}


def make(task, seed):
    """(processed full-resolution prediction, label) of one batch"""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B, CH[task], S, S, generator=g)
    if task in ("semseg", "human_parts"):
        lab = torch.randint(0, CH[task], (B, 1, S, S), generator=g).float()
        lab[torch.rand(B, 1, S, S, generator=g) < 0.07] = 255.0
    elif task == "normals":
        lab = F.normalize(torch.randn(B, 3, S, S, generator=g), dim=1)
        lab[torch.rand(B, 3, S, S, generator=g) < 0.03] = 255.0
    elif task == "sal":
        lab = (torch.rand(B, 1, S, S, generator=g) < 0.3).float()
        lab[torch.rand(B, 1, S, S, generator=g) < 0.03] = 255.0
    elif task == "depth":
        out = 3.0 + 0.8 * out
        lab = 0.5 + 9 * torch.rand(B, 1, S, S, generator=g)
        lab[torch.rand(B, 1, S, S, generator=g) < 0.07] = 255.0
    else:
        lab = (torch.rand(B, 1, S, S, generator=g) < 0.1).float()
    return get_output(out, task), lab


def state(m):
    """everything a meter accumulates, as comparable host values"""
    st = {"counts": None if m.counts is None else m.counts.clone(), "sums": None if m.sums is None else m.sums.clone()}
    if hasattr(m, "per_image"):
        st["per_image"] = [p.clone() for p in m.per_image]
        st["per_image_valid"] = list(m.per_image_valid)
    if hasattr(m, "n"):
        st["n"] = m.n
        st["n_dev"] = m.n_dev
    return st


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            assert len(x) == len(y), k
            for p, q in zip(x, y):
                assert (p is None and q is None) or torch.equal(p, q), k
        elif isinstance(x, torch.Tensor):
            assert torch.equal(x, y), (k, x, y)
        else:
            assert x == y, (k, x, y)


def same_score(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k], float), np.asarray(b[k], float), equal_nan=True), (k, a[k], b[k])


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("task", ALL6)
def test_update_valid_is_update_of_the_labelled_sub_batch(task, mask):
    flags = torch.tensor(MASKS[mask], dtype=torch.uint8)
    idx = torch.nonzero(flags).reshape(-1)
    got, want = get_single_task_meter(task), get_single_task_meter(task)
    for i in range(2):  # two batches: the state accumulates
        pred, lab = make(task, seed=10 * i + ALL6.index(task))
        lab_poisoned = lab.clone()
        lab_poisoned[flags == 0] = float("nan")  # what an unlabelled sample's label may hold
        got.update(pred, lab_poisoned, flags)
        want.update(pred.index_select(0, idx), lab.index_select(0, idx))
    same(state(got), state(want))
    same_score(got.get_score(verbose=False), want.get_score(verbose=False))


@pytest.mark.parametrize("task", ALL6)
def test_all_ones_equals_none_and_empty_changes_nothing(task):
    pred, lab = make(task, seed=3)
    a, b = get_single_task_meter(task), get_single_task_meter(task)
    a.update(pred, lab, torch.ones(B, dtype=torch.uint8))
    b.update(pred, lab)
    same(state(a), state(b))
    before = state(a)
    a.update(pred, torch.full_like(lab, float("nan")), torch.zeros(B, dtype=torch.uint8))
    same(state(a), before)
    fresh = get_single_task_meter(task)
    fresh.update(pred, lab, torch.zeros(B, dtype=torch.uint8))  # also on a meter that has seen nothing
    same(state(fresh), state(get_single_task_meter(task)))
    with pytest.raises(RuntimeError, match="one flag per sample"):
        a.update(pred, lab, torch.ones(B + 1, dtype=torch.uint8))


def test_saliency_unlabelled_rows_do_not_enter_maxf_or_miou():
    """an unlabelled image's label is all zero here and its prediction all negative: scored, it would be a perfect Jaccard of 1 at
    every threshold (nothing there, nothing found) and move mIoU"""
    pred, lab = make("sal", seed=5)
    pred, lab = pred.clone(), lab.clone()
    pred[1], lab[1] = 0.0, 0.0
    flags = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
    idx = torch.nonzero(flags).reshape(-1)
    masked, sub, everything = (get_single_task_meter("sal") for _ in range(3))
    masked.update(pred, lab, flags)
    sub.update(pred[idx], lab[idx])
    everything.update(pred, lab)
    assert sum(p.shape[0] for p in masked.per_image) == 3
    sm, ss, se = (m.get_score(verbose=False) for m in (masked, sub, everything))
    assert sm["maxF"] == ss["maxF"] and sm["mIoU"] == ss["mIoU"] and sm["Beta maxF"] == ss["Beta maxF"]
    assert se["mIoU"] > sm["mIoU"]  # the row that must stay out
    # the fused route's bookkeeping: a zero row next to its flag is dropped by get_score()
    m = get_single_task_meter("sal")
    m.update(pred[idx], lab[idx])
    rows = m.per_image[0]
    padded = torch.zeros(B, 15, 3, dtype=rows.dtype)
    padded[idx] = rows
    m.per_image, m.per_image_valid = [padded], [flags.clone()]
    same_score(m.get_score(verbose=False), ss)


def test_performance_meter_update_valid_dict():
    preds, labs = {}, {}
    for k, t in enumerate(ALL6):
        preds[t], labs[t] = make(t, seed=20 + k)
    valid = {"semseg": torch.tensor([1, 0, 1, 0], dtype=torch.uint8), "sal": torch.tensor([0, 0, 0, 1], dtype=torch.uint8),
             "depth": torch.zeros(B, dtype=torch.uint8)}  # the other three tasks: no entry, labelled everywhere
    got, want = PerformanceMeter(ALL6), PerformanceMeter(ALL6)
    got.update(preds, labs, valid)
    for t in ALL6:
        if t in valid:
            idx = torch.nonzero(valid[t]).reshape(-1)
            if idx.numel():
                want.meters[t].update(preds[t].index_select(0, idx), labs[t].index_select(0, idx))
        else:
            want.meters[t].update(preds[t], labs[t])
        same(state(got.meters[t]), state(want.meters[t]))
    assert got.meters["depth"].counts is None
    plain, none = PerformanceMeter(ALL6), PerformanceMeter(ALL6)
    plain.update(preds, labs)
    none.update(preds, labs, None)
    for t in ALL6:
        same(state(plain.meters[t]), state(none.meters[t]))
