"""CPU tests of the validation API (mtlora_amd/evaluation.py, the edge / depth losses and inputs of mtl_harness) against
tests/golden/eval_meters.pt, which tests/golden/make_golden_eval.py recorded from the REAL reference meters
(evaluation/evaluate_utils.py PerformanceMeter + get_output) and losses (mtl_loss_schemes.get_loss) on the same inputs.

Integer-derived scores (the segmentation jaccards and mIoU) must match exactly; float scores to 1e-6 relative: fp32 meters
against fp32 meters on the same CPU, the margin is for summation order only (the golden side sums fp32 terms in fp32 after a
masked_select, this side sums the same fp32 terms in fp64 in place).
"""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "eval_meters.pt")
RTOL = 1e-6

KEYS = {"semseg": {"mIoU", "jaccards_all_categs"}, "human_parts": {"mIoU", "jaccards_all_categs"},
        "normals": {"mean", "rmse", "mean_v2", "rmse_v2"}, "sal": {"maxF", "Beta maxF", "mIoU"},
        "depth": {"rmse", "log_rmse"}, "edge": {"loss"}}


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


def _batches(gold):
    for b in gold["batches"]:
        yield {t: v.float() for t, v in b["out"].items()}, {t: v.float() for t, v in b["lab"].items()}


def _close(a, b, rtol=RTOL):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


def _meter_scores(gold, tasks):
    from mtlora_amd.evaluation import PerformanceMeter, get_output
    meter = PerformanceMeter(tasks, "PASCALContext")
    for out, lab in _batches(gold):
        meter.update({t: get_output(out[t], t) for t in tasks}, {t: lab[t] for t in tasks})
    return meter, meter.get_score(verbose=False)


def test_meters_match_the_reference_meters(gold):
    tasks = gold["tasks"]
    assert set(tasks) == set(KEYS)
    _, got = _meter_scores(gold, tasks)
    assert set(got) == set(tasks)
    for t in tasks:
        ref = gold["scores"][t]
        assert set(got[t]) == KEYS[t] == set(ref), (t, set(got[t]))
        for k, v in ref.items():
            if t in ("semseg", "human_parts"):  # ratios of integer counts: exact
                if k == "jaccards_all_categs":
                    assert list(got[t][k]) == list(v), t
                else:
                    assert float(got[t][k]) == v, (t, k)
            else:
                print(t, k, float(got[t][k]), v, abs(float(got[t][k]) - v) / abs(v))
                assert _close(float(got[t][k]), v), (t, k, float(got[t][k]), v)
    # the reference's quirk, kept: both normals meters report the mean as rmse
    assert got["normals"]["rmse"] == got["normals"]["mean"] and got["normals"]["rmse_v2"] == got["normals"]["mean_v2"]


def test_saliency_image_without_positives_scores_jaccard_one(gold):
    """batch 1, image 1 has no positive pixel and no prediction above any threshold: jaccard.py:27-28 returns 1 there"""
    from mtlora_amd.evaluation import SaliencyMeter, get_output
    out, lab = list(_batches(gold))[1]
    assert (lab["sal"][1] == 0).all()
    m = SaliencyMeter()
    m.update(get_output(out["sal"], "sal"), lab["sal"])
    per = m.per_image[0]
    assert (per[1] == 0).all()  # tp = fp = fn = 0 at all 15 thresholds
    single = SaliencyMeter()
    single.update(get_output(out["sal"][1:].repeat(2, 1, 1, 1), "sal"), lab["sal"][1:].repeat(2, 1, 1, 1))
    assert single.get_score(verbose=False)["mIoU"] == 1.0


def test_meter_reset_and_accumulation(gold):
    tasks = gold["tasks"]
    meter, first = _meter_scores(gold, tasks)
    meter.reset()
    from mtlora_amd.evaluation import get_output
    for out, lab in _batches(gold):
        meter.update({t: get_output(out[t], t) for t in tasks}, {t: lab[t] for t in tasks})
    again = meter.get_score(verbose=False)
    for t in tasks:
        for k in first[t]:
            assert again[t][k] == first[t][k], (t, k)
    # one batch alone scores differently from three: update() accumulates
    meter.reset()
    out, lab = next(_batches(gold))
    meter.update({t: get_output(out[t], t) for t in tasks}, {t: lab[t] for t in tasks})
    assert meter.get_score(verbose=False)["depth"]["rmse"] != first["depth"]["rmse"]


def test_update_low_on_cpu_takes_the_plain_path(gold):
    """update_low with CPU tensors == update(get_output(interpolate(low))), and it returns the task losses"""
    from mtlora_amd.evaluation import PerformanceMeter, get_output
    from mtlora_amd.mtl_harness import task_loss
    import torch.nn.functional as F
    tasks = gold["tasks"]
    out, lab = next(_batches(gold))
    low = {t: out[t][:, :, ::4, ::4].permute(0, 2, 3, 1).contiguous() for t in tasks}
    a, b = PerformanceMeter(tasks), PerformanceMeter(tasks)
    losses = a.update_low(low, lab)
    up = {t: F.interpolate(low[t].permute(0, 3, 1, 2), lab[t].shape[-2:], mode="bilinear") for t in tasks}
    b.update({t: get_output(up[t], t) for t in tasks}, lab)
    sa, sb = a.get_score(verbose=False), b.get_score(verbose=False)
    for t in tasks:
        assert sa[t] == sb[t], t
        assert torch.equal(losses[t], task_loss(t, up[t], lab[t])), t


@pytest.mark.parametrize("task", ["edge", "depth", "semseg", "human_parts", "normals", "sal"])
def test_task_loss_matches_the_reference_loss(gold, task):
    from mtlora_amd.mtl_harness import task_loss
    for (out, lab), ref in zip(_batches(gold), gold["losses"]):
        got = float(task_loss(task, out[task], lab[task]))
        print(task, got, ref[task], abs(got - ref[task]) / abs(ref[task]))
        assert _close(got, ref[task]), (task, got, ref[task])


def test_calculate_multi_task_performance(gold):
    from mtlora_amd.evaluation import calculate_multi_task_performance
    tasks = [t for t in gold["tasks"] if t != "edge"]
    _, got = _meter_scores(gold, tasks)
    v = calculate_multi_task_performance(got, gold["single"])
    assert _close(float(v), gold["multi_task_performance"]), (v, gold["multi_task_performance"])
    with pytest.raises(AssertionError):
        calculate_multi_task_performance(got, {"semseg": gold["single"]["semseg"]})


def test_get_output_shapes_and_errors():
    from mtlora_amd.evaluation import get_output
    x = torch.randn(2, 3, 5, 4)
    n = get_output(x, "normals")
    assert n.shape == (2, 5, 4, 3) and float(n.min()) >= 0 and float(n.max()) <= 255
    assert get_output(torch.randn(2, 7, 5, 4), "human_parts").shape == (2, 5, 4)
    assert get_output(torch.randn(2, 1, 5, 4), "sal").shape == (2, 5, 4)
    assert get_output(torch.randn(2, 1, 5, 4), "depth").shape == (2, 5, 4, 1)
    with pytest.raises(ValueError):
        get_output(x, "nothing")


def test_synthetic_batch_and_model_for_the_nyud_task_set():
    from mtlora_amd import mtl_harness as H
    img, tg = H.synthetic_batch(2, 32, H.NYUD4, seed=3, num_outputs=H.NYUD_NUM_OUTPUT)
    assert img.shape == (2, 3, 32, 32) and set(tg) == set(H.NYUD4)
    e = tg["edge"]
    assert e.shape == (2, 1, 32, 32) and set(e.unique().tolist()) <= {0.0, 1.0} and 0.02 < float(e.mean()) < 0.25
    s = tg["semseg"]
    assert float(s[s != 255].max()) > 21 and float(s[s != 255].max()) < 40
    # the inputs of the existing task sets do not move: same draws as before for the four PASCAL tasks
    _, a = H.synthetic_batch(1, 16, H.PASCAL4, seed=5)
    _, b = H.synthetic_batch(1, 16, H.PASCAL4 + ("edge",), seed=5)
    for t in H.PASCAL4:
        assert torch.equal(a[t], b[t])
    crit = H.MultiTaskLoss(H.NYUD4)
    assert crit.loss_weights["edge"] == 50.0 and set(H.NYUD4) <= set(crit.FUSED_KIND)
    pred = {t: torch.randn(2, H.NYUD_NUM_OUTPUT.get(t, H.num_output(t)), 32, 32) for t in H.NYUD4}
    total, per = crit(pred, tg)
    assert torch.isfinite(total) and set(per) == set(H.NYUD4) | {"total"}
