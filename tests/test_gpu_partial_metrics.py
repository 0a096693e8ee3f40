"""Partially labelled batches at the measuring end, on the GPU (run on an MI355X: -m gpu): mtlora_upsample_metrics_valid
(csrc/metrics.hip) against the unchanged unmasked launch on the gathered sub-batch (counts exactly, floats at FLOAT_RTOL -- the
number of partials differs, the per-pixel arithmetic does not), bit for bit against it where every sample is labelled, and
against the fp64 restatement of tests/test_gpu_eval.py; the unlabelled samples' prediction and label are never read (NaN / Inf
in them change no bit); a captured launch follows the flag buffer; validate_step(valid=), validate() and
train_step(performance_meter=, valid=) on the small model of tests/test_gpu_eval.py.

Seeds of the fp64 comparison (geometry FP64_GEOM, every non-empty mask, both dtypes): the ambiguous share of the SUB-BATCH
inputs was computed with reference() on the CPU for every case before the seeds were fixed; the largest is 3.6e-4 (sal, bf16,
mask "alternating"), the bound AMBIGUOUS_SHARE = 1e-3.  check() asserts it again on every run.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_eval import (ALL6, AMBIGUOUS_SHARE, CH, FLOAT_RTOL, KIND_OF, _small, _warm_bn, check, dev, make_case,  # noqa: F401
                           quantise, reference)

pytestmark = pytest.mark.gpu

GEOM = [(4, 26, 30, 4),   # non-square, partial column and row tiles
        (4, 33, 70, 1),   # scale 1, 64-column tiles
        (3, 10, 21, 8)]   # the heads' scale, a width off the tile, several tiles per sample
FP64_GEOM = GEOM[0]
ERR_NULL = -4  # include/mtlora_hip.h


def masks_of(B):
    return {"first": [1] + [0] * (B - 1), "last": [0] * (B - 1) + [1], "alternating": [(b + 1) % 2 for b in range(B)],
            "all": [1] * B, "empty": [0] * B}


def seed_of(task, h, w, S):
    return 1000 + 31 * ALL6.index(task) + 7 * h + w + S


def bits64(t):
    return t.detach().contiguous().view(torch.int64).cpu()


def prefill(n):
    """a non-zero pattern for `counts`: the launch ADDS, so a delta shows what it added and where"""
    return (torch.arange(max(n, 1), dtype=torch.int64) * 3 + 7).to(dev())


def poison(low, lab, off):
    """NaN and +-Inf (what the non-finite tests feed this kernel) into the samples `off`"""
    lo2, la2 = low.clone(), lab.clone()
    for k, b in enumerate(off):
        lo2[b] = (float("nan"), float("inf"), -float("inf"))[k % 3]
        la2[b] = (float("inf"), float("nan"), -float("inf"))[k % 3]
    return lo2, la2


def sal_rows(counts, B):
    return counts[57:57 + 45 * B].view(B, 45)


def close(a, b, what):
    a, b = a.double().cpu(), b.double().cpu()
    for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        e = abs(x - y) / max(abs(y), 1e-300)
        print(f"{what}: float {i} masked {x:.9g} sub-batch {y:.9g} rel {e:.3e}")
        assert e <= FLOAT_RTOL, (what, i, x, y, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,h,w,S", GEOM)
@pytest.mark.parametrize("task", ALL6)
def test_masked_launch(task, B, h, w, S, dtype):
    from mtlora_amd import functional as Fn
    kind = KIND_OF[task]
    low, lab = make_case(task, B, h, w, S, seed=seed_of(task, h, w, S))
    low_q = quantise(low, dtype)
    lowd, labd = low_q.to(dev()), lab.to(dev())
    ni, _ = Fn.upsample_metrics_sizes(kind, B, h, w, CH[task], S)

    for name, mask in masks_of(B).items():
        what = f"{task} {B}x{h}x{w} S{S} {dtype} {name}"
        valid = torch.tensor(mask, dtype=torch.uint8, device=dev())
        on = [b for b in range(B) if mask[b]]
        off = [b for b in range(B) if not mask[b]]
        base = prefill(ni)
        counts, sums = Fn.upsample_metrics(kind, lowd, labd, S, counts=base.clone(), valid=valid)
        delta = (counts - base)[:ni]
        assert sums.dtype == torch.float64 and sums.shape == (Fn.METRIC_FLOATS[kind],)

        if not on:
            # 4. no labelled sample: counts unchanged, every float +0.0
            assert ni == 0 or int(delta.abs().sum()) == 0, what
            assert int(bits64(sums).abs().max()) == 0 and torch.isfinite(sums).all(), (what, sums)
            lo2, la2 = poison(lowd, labd, off)
            c2, s2 = Fn.upsample_metrics(kind, lo2, la2, S, counts=base.clone(), valid=valid)
            assert torch.equal(c2, base) and int(bits64(s2).abs().max()) == 0, what
            continue

        # 1. against the unmasked launch on the gathered sub-batch
        idx = torch.tensor(on, device=dev())
        c_sub, s_sub = Fn.upsample_metrics(kind, lowd.index_select(0, idx), labd.index_select(0, idx), S)
        if kind == "saliency":
            assert torch.equal(delta[:57], c_sub[:57]), what
            assert torch.equal(sal_rows(delta, B)[on], sal_rows(c_sub, len(on))), what
            if off:
                assert int(sal_rows(delta, B)[off].abs().sum()) == 0, what
            assert int(sal_rows(delta, B)[on].sum()) > 0
        elif ni:
            assert torch.equal(delta, c_sub[:ni]), (what, delta, c_sub)
            assert int(delta.sum()) > 0
        close(sums, s_sub, what)

        # ... and, at one geometry, against the fp64 restatement of the sub-batch
        if (B, h, w, S) == FP64_GEOM:
            ref = reference(task, low_q[on], lab[on], S)
            got = delta.cpu().numpy()
            if kind == "saliency":
                got = np.concatenate([got[:57], sal_rows(delta, B)[on].reshape(-1).cpu().numpy()])
            check(what, got, sums.cpu().tolist(), ref)

        # 2. every sample labelled: the bits of the unmasked launch
        if not off:
            c_old, s_old = Fn.upsample_metrics(kind, lowd, labd, S, counts=base.clone())
            assert torch.equal(counts, c_old), what
            assert torch.equal(bits64(sums), bits64(s_old)), (what, sums, s_old)
            continue

        # 3. neither the prediction nor the label of an unlabelled sample is read
        lo2, la2 = poison(lowd, labd, off)
        c2, s2 = Fn.upsample_metrics(kind, lo2, la2, S, counts=base.clone(), valid=valid)
        assert torch.equal(c2, counts), what
        assert torch.equal(bits64(s2), bits64(sums)), (what, s2, sums)
        assert torch.isfinite(s2).all()


@pytest.mark.parametrize("task", ["semseg", "normals", "sal", "depth", "edge"])
def test_captured_launch_follows_the_valid_buffer(task):
    """ONE capture per kind on a single stream; the flags are rewritten between replays and `counts` is zeroed outside the graph"""
    from mtlora_amd import functional as Fn
    B, h, w, S = GEOM[2]
    kind = KIND_OF[task]
    low, lab = make_case(task, B, h, w, S, seed=seed_of(task, h, w, S))
    lowd, labd = low.to(dev()), lab.to(dev())
    ni, _ = Fn.upsample_metrics_sizes(kind, B, h, w, CH[task], S)
    valid = torch.ones(B, dtype=torch.uint8, device=dev())
    counts = torch.zeros(max(ni, 1), dtype=torch.int64, device=dev())
    Fn.upsample_metrics(kind, lowd, labd, S, counts=counts, valid=valid)  # (warm: workspaces, the threshold table)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (captures on one side stream)
        _, sums = Fn.upsample_metrics(kind, lowd, labd, S, counts=counts, valid=valid)
    ms = masks_of(B)
    for name in ("alternating", "first", "empty", "last", "all"):
        valid.copy_(torch.tensor(ms[name], dtype=torch.uint8))
        counts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        c_eager, s_eager = Fn.upsample_metrics(kind, lowd, labd, S, valid=torch.tensor(ms[name], dtype=torch.uint8, device=dev()))
        assert torch.equal(counts[:ni], c_eager[:ni]), (task, name)
        assert torch.equal(bits64(sums), bits64(s_eager)), (task, name, sums, s_eager)
    assert float(sums[0]) != 0.0  # (the last replay: every sample labelled)


def test_argument_checks():
    from mtlora_amd import _lib as L
    from mtlora_amd import functional as Fn
    lib = L.lib()
    B, h, w, S = 2, 8, 8, 4
    low = torch.zeros(B, h, w, 21, device=dev())
    lab = torch.zeros(B, 1, h * S, w * S, device=dev())
    stat = torch.ones(2, device=dev())
    ni, nfp = Fn.upsample_metrics_sizes("softmax", B, h, w, 21, S)
    counts = torch.full((ni,), 5, dtype=torch.int64, device=dev())
    part = torch.full((nfp,), -7.0, device=dev())
    valid = torch.ones(B, dtype=torch.uint8, device=dev())
    P = ctypes.c_void_p

    def call(v=valid.data_ptr(), lo=low.data_ptr(), dtype=L.F32, nb=B):
        return lib.mtlora_upsample_metrics_valid(0, P(lo), P(lab.data_ptr()), P(v), P(stat.data_ptr()), P(counts.data_ptr()),
                                                 P(part.data_ptr()), nb, h, w, 21, S, dtype, 255.0, L.stream_ptr())

    assert call(v=0) == ERR_NULL and call(lo=0) == ERR_NULL
    assert call(dtype=L.F16) == -1  # as the unmasked entry
    assert call(v=0, nb=0) == 0     # B == 0: nothing to do
    torch.cuda.synchronize()
    assert (counts == 5).all() and (part == -7.0).all()  # a rejected call launches nothing
    with pytest.raises(RuntimeError, match="valid lives on"):
        Fn.upsample_metrics("softmax", low, lab, S, valid=torch.ones(B, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="valid must be a uint8"):
        Fn.upsample_metrics("softmax", low, lab, S, valid=torch.ones(B + 1, dtype=torch.uint8, device=dev()))
    with pytest.raises(RuntimeError, match="valid must be a uint8"):
        Fn.upsample_metrics("softmax", low, lab, S, valid=torch.ones(B, dtype=torch.bool, device=dev()))
    torch.cuda.synchronize()
    assert (counts == 5).all() and (part == -7.0).all()


# ------------------------------------------------------------------------------------------------
# harness level: the small model of tests/test_gpu_eval.py (224 px: 28 x 28 head outputs, scale 8), B = 4
# ------------------------------------------------------------------------------------------------
PASCAL4 = ("semseg", "normals", "sal", "human_parts")
MASK_PASCAL4 = {"semseg": [1, 0, 1, 0], "normals": [0, 0, 0, 1], "sal": [1, 1, 0, 1], "human_parts": [0, 1, 1, 0]}
# (semseg has no entry: labelled everywhere; edge wholly unlabelled)
MASK_ALL6 = {"human_parts": [1, 0, 0, 0], "normals": [0, 1, 1, 1], "sal": [0, 1, 0, 1], "depth": [1, 1, 0, 0], "edge": [0, 0, 0, 0]}


def meter_state(meter, t):
    """(counts in the kernel's layout over the labelled images, float sums without the loss) of one task's meter"""
    m = meter.meters[t]
    if m.counts is None:
        return None
    if t == "edge":
        n = m.n + (0 if m.n_dev is None else int(m.n_dev.item()))
        return np.zeros(0, np.int64), [m.sums[0].item() / n] if n else []
    c = m.counts.cpu().numpy()
    if t == "sal":
        c = np.concatenate([c[:57], m._per_image_rows().reshape(-1)])
    s = m.sums.cpu().tolist()
    return c, (s if t in ("normals", "depth") else [])


@pytest.mark.parametrize("tasks,masks", [(PASCAL4, MASK_PASCAL4), (tuple(ALL6), MASK_ALL6)], ids=["pascal4", "all6"])
def test_validate_step_valid_vs_portable_route(tasks, masks):
    """validate_step(valid=) against meter.update(get_output(F.interpolate(low)), gt, valid) and task_loss(..., valid) on the
    model's own low-resolution outputs, fp32: both meter states within the bound of
    test_gpu_eval.py::test_validate_step_vs_full_resolution_route of the fp64 restatement of the labelled sub-batch, the
    per-task losses at its 1e-4"""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter, get_output
    B = 4
    model = _warm_bn(_small(tasks), tasks)
    if "depth" in tasks:  # input condition of the depth meter: predictions away from the clamp at 0
        with torch.no_grad():
            model.decoders.decoders["depth"].last_layer[3].bias.fill_(3.0)
    crit = H.MultiTaskLoss(tasks)
    img, tg, valid = H.synthetic_batch(B, 224, tasks, seed=31, device=dev(), valid=masks)
    fused, plain = PerformanceMeter(tasks), PerformanceMeter(tasks)
    total, per = H.validate_step(model, crit, fused, img, tg, amp_dtype=None, valid=valid)
    assert model.training and set(per) == set(tasks) | {"total"}
    model.eval()
    with torch.no_grad():
        low = model(img, upsample=False)
    model.train()
    up = {t: F.interpolate(low[t].float().permute(0, 3, 1, 2), scale_factor=8, mode="bilinear") for t in tasks}
    plain.update({t: get_output(up[t], t) for t in tasks}, tg, valid)
    want_total = 0.0
    for t in tasks:
        on = [b for b in range(B) if masks.get(t, [1] * B)[b]]
        want = H.task_loss(t, up[t], tg[t], valid.get(t))
        want_total += crit.loss_weights[t] * want.item()
        print(t, "loss", per[t].item(), want.item())
        assert abs(per[t].item() - want.item()) <= 1e-4 * max(abs(want.item()), 1e-12), (t, per[t].item(), want.item())
        if not on:  # a wholly unlabelled task: nothing counted, a loss of exactly 0
            assert per[t].item() == 0.0 and plain.meters[t].counts is None
            m = fused.meters[t]
            assert int(m.counts.abs().sum()) == 0 and float(m.sums.abs().sum()) == 0.0
            if t == "edge":
                assert int(m.n_dev.item()) == 0 and m.n == 0
            continue
        ref = reference(t, low[t][on].cpu(), tg[t][on].cpu(), 8)
        ref = (ref[0], ref[1], [0.0] + list(ref[2][1:]), ref[3])
        for name, meter in (("fused", fused), ("plain", plain)):
            c, s = meter_state(meter, t)
            check(f"validate_step(valid=) {name} {t}", c, [0.0] + s, ref)
    assert abs(total.item() - want_total) <= 1e-4 * abs(want_total), (total.item(), want_total)
    if "edge" not in masks:  # (get_score needs a labelled sample per task)
        sf, sp = fused.get_score(verbose=False), plain.get_score(verbose=False)
        for t in tasks:
            assert set(sf[t]) == set(sp[t]), t


def test_validate_takes_two_and_three_tuples():
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter
    tasks = PASCAL4
    model = _warm_bn(_small(tasks), tasks).eval()
    crit = H.MultiTaskLoss(tasks)
    b0 = H.synthetic_batch(4, 224, tasks, seed=41, device=dev())
    b1 = H.synthetic_batch(4, 224, tasks, seed=42, device=dev(), valid=MASK_PASCAL4)
    b2 = H.synthetic_batch(4, 224, tasks, seed=43, device=dev(), valid={"sal": [0, 0, 1, 1]})
    assert len(b0) == 2 and len(b1) == 3
    scores, loss = H.validate(model, [b0, b1, b2], amp_dtype=None)
    meter = PerformanceMeter(tasks)
    losses = [H.validate_step(model, crit, meter, b0[0], b0[1], None)[0],
              H.validate_step(model, crit, meter, b1[0], b1[1], None, b1[2])[0],
              H.validate_step(model, crit, meter, b2[0], b2[1], None, valid=b2[2])[0]]
    want = meter.get_score(verbose=False)
    assert loss == float(sum(l.double() for l in losses)) / 3 and math.isfinite(loss)
    for t in tasks:
        assert set(scores[t]) == set(want[t])
        for k in want[t]:
            assert np.array_equal(np.asarray(scores[t][k], float), np.asarray(want[t][k], float)), (t, k)
    assert len(meter.meters["sal"]._per_image_rows()) == 4 + 3 + 2
    with pytest.raises(ValueError, match="a batch is"):
        H.validate(model, [(b0[0],)], amp_dtype=None)


def test_update_low_valid_does_not_synchronise():
    """PerformanceMeter.update_low(low, gt, valid) under torch.cuda.set_sync_debug_mode("error"), after one warm call (workspaces,
    the saliency threshold table's one host-to-device copy)"""
    from mtlora_amd.evaluation import PerformanceMeter
    B, h, w, S = 3, 10, 21, 8
    low, lab = {}, {}
    for k, t in enumerate(ALL6):
        lo, la = make_case(t, B, h, w, S, seed=k)
        low[t], lab[t] = lo.to(dev()), la.to(dev())
    valid = {t: torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev()) for t in ALL6 if t != "semseg"}
    meter = PerformanceMeter(ALL6)
    meter.update_low(low, lab, valid)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = meter.update_low(low, lab, valid)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(math.isfinite(v.item()) for v in losses.values())
    assert meter.get_score(verbose=False)["edge"]["loss"] > 0.0


def test_train_step_with_a_performance_meter():
    """train_step(performance_meter=, valid=): loss, gradient norm and every trainable parameter after the step bit-equal to the
    step without a meter (two identical models, dropout and DropPath off), and the meter holds what update_low gives on the
    low-resolution outputs of a train-mode forward of a third identical model"""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter
    tasks = PASCAL4
    img, tg, valid = H.synthetic_batch(4, 224, tasks, seed=51, device=dev(), valid=MASK_PASCAL4)

    def fresh():
        return H.build_model(img_size=224, tasks=tasks, r_shared=16, r_task=4, seed=0, drop_path_rate=0.0,
                             dropout=0.0).to(dev()).train()

    out = []
    meter = PerformanceMeter(tasks)
    for pm in (None, meter):
        model = fresh()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3)
        loss, norm = H.train_step(model, crit, opt, img, tg, amp_dtype=None, valid=valid, performance_meter=pm)
        torch.cuda.synchronize()
        out.append((loss.clone(), norm.clone(), {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}))
    (l0, n0, p0), (l1, n1, p1) = out
    assert math.isfinite(l0.item()) and math.isfinite(n0.item())
    assert torch.equal(l0, l1) and torch.equal(n0, n1), (l0.item(), l1.item(), n0.item(), n1.item())
    assert set(p0) == set(p1) and len(p0) > 50
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    model = fresh()
    low = {t: v.detach() for t, v in model(img, upsample=False).items()}
    want = PerformanceMeter(tasks)
    want.update_low(low, tg, valid)
    for t in tasks:
        a, b = meter.meters[t], want.meters[t]
        assert torch.equal(a.counts, b.counts) and int(a.counts.sum()) > 0, t
        assert torch.equal(a.sums, b.sums), t
    assert np.array_equal(meter.meters["sal"]._per_image_rows(), want.meters["sal"]._per_image_rows())
    sa, sb = meter.get_score(verbose=False), want.get_score(verbose=False)
    for t in tasks:
        for k in sb[t]:
            assert np.array_equal(np.asarray(sa[t][k], float), np.asarray(sb[t][k], float)), (t, k)
