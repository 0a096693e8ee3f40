"""CPU tests of partially labelled batches (DESIGN.md "Partially labelled batches"): the plain-torch definitions
(mtl_harness.task_loss(valid=), functional.upsample_loss_valid_torch) against tests/golden/partial_labels.pt, which
tests/golden/make_golden_partial.py recorded from the REAL reference criteria (mtl_loss_schemes.get_loss) applied in fp64 to
the index-selected sub-batch (pred[V], gt[V]); the wire-batch plumbing of data.py; the header and the host-side argument checks
of the two new library entries.

Tolerance: RTOL of tests/test_cpu_eval.py (1e-6 relative) for the loss values.  The fixture records each gradient compactly
(eight +-1 projections, Euclidean norm, largest magnitude); the same figure holds for them, the projections relative to the norm.
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "partial_labels.pt")
RTOL = 1e-6  # tests/test_cpu_eval.py
KIND = {"semseg": ("softmax", None), "human_parts": ("softmax", None), "normals": ("normals", None), "sal": ("balanced_bce", None),
        "depth": ("l1_masked", None), "edge": ("balanced_bce", 0.95)}
TASKS = list(KIND)


@pytest.fixture(scope="module")
def built_lib():
    from mtlora_amd.csrc.build import build
    return build(verbose=False)


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_partial", os.path.join(ROOT, "tests", "golden", "make_golden_partial.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


def _grad_errors(grad, mask, rec):
    """a (B, ...) gradient against the fixture's compact record of d loss / d pred[V] (make_golden_partial.compact): the largest
    projection error and the error of the largest magnitude, both relative to the recorded scale; the rows outside V must be 0"""
    G = _generator()
    on = torch.tensor(mask, dtype=torch.bool)
    assert (grad[~on] == 0).all()
    got = G.compact(grad[on])
    e_proj = max(abs(a - b) for a, b in zip(got["proj"], rec["proj"])) / rec["l2"]
    return max(e_proj, abs(got["l2"] - rec["l2"]) / rec["l2"], abs(got["max"] - rec["max"]) / rec["max"])


def test_fixture_is_what_the_generator_describes(gold):
    assert gold["tasks"] == TASKS or set(gold["tasks"]) == set(TASKS)
    assert [c["mask"] for c in gold["cases"]] == [[1, 1, 1], [1, 0, 1], [0, 0, 1]]
    for t in TASKS:
        assert gold["out"][t].shape[0] == 3 and tuple(gold["out"][t].shape[-2:]) == (16, 16)
    assert os.path.getsize(GOLD) < 64 << 10
    P = _generator().probes(4096)
    assert P.shape == (8, 4096) and set(P.unique().tolist()) == {-1.0, 1.0} and float(P.mean(1).abs().max()) < 0.05


@pytest.mark.parametrize("task", TASKS)
def test_task_loss_valid_matches_the_reference_on_the_sub_batch(gold, task):
    from mtlora_amd.mtl_harness import task_loss
    for case in gold["cases"]:
        valid = torch.tensor(case["mask"], dtype=torch.uint8)
        out = gold["out"][task].float().requires_grad_(True)
        lab = gold["lab"][task].float()
        lab_garbage = lab.clone()
        lab_garbage[valid == 0] = float("nan")  # an unlabelled sample's label is never read
        got = task_loss(task, out, lab_garbage, valid)
        got.backward()
        ref = case["loss"][task]
        e = abs(got.item() - ref) / abs(ref)
        g = _grad_errors(out.grad, case["mask"], case["grad"][task])
        print(task, case["mask"], got.item(), ref, e, g)
        assert e <= RTOL, (task, case["mask"], got.item(), ref)
        assert g <= RTOL, (task, case["mask"], g)
        assert (out.grad[valid == 0] == 0).all()
    # no flags and all-ones flags: the value of the unchanged call
    out, lab = gold["out"][task].float(), gold["lab"][task].float()
    assert torch.equal(task_loss(task, out, lab, torch.ones(3, dtype=torch.uint8)), task_loss(task, out, lab))


@pytest.mark.parametrize("task", TASKS)
def test_upsample_loss_valid_torch_matches_the_reference_in_fp64(gold, task):
    """scale 1 is the identity upsample, so the full-resolution fixture pins the definition itself; in fp64"""
    from mtlora_amd import functional as Fn
    kind, pw = KIND[task]
    for case in gold["cases"]:
        valid = torch.tensor(case["mask"], dtype=torch.uint8)
        low = gold["out"][task].double().permute(0, 2, 3, 1).contiguous()
        lab = gold["lab"][task].double()
        low[valid == 0] = float("inf")  # neither the prediction nor the label of an unlabelled sample is read
        lab[valid == 0] = float("nan")
        low.requires_grad_(True)
        got = Fn.upsample_loss_valid_torch(kind, low, lab, 1, valid, pos_weight=pw)
        assert got.dtype == torch.float64
        got.backward()
        ref = case["loss"][task]
        e = abs(got.item() - ref) / abs(ref)
        g = _grad_errors(low.grad.permute(0, 3, 1, 2), case["mask"], case["grad"][task])
        print(task, case["mask"], got.item(), ref, e, g)
        assert e <= RTOL and g <= RTOL, (task, case["mask"], e, g)


def test_upsample_loss_valid_torch_is_the_selected_sub_batch():
    """at a real scale: the definition equals the criterion on interpolate(low[V]) (autograd through the selection)"""
    from mtlora_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    low = torch.randn(3, 5, 9, 1, generator=g, dtype=torch.float64, requires_grad=True)
    lab = torch.rand(3, 1, 20, 36, generator=g, dtype=torch.float64) * 10
    valid = torch.tensor([1, 0, 1], dtype=torch.uint8)
    got = Fn.upsample_loss_valid_torch("l1_masked", low, lab, 4, valid)
    sel = torch.tensor([0, 2])
    up = F.interpolate(low[sel].permute(0, 3, 1, 2), scale_factor=4, mode="bilinear")
    ref = (up - lab[sel]).abs().mean()
    assert abs(got.item() - float(ref)) <= 1e-12 * abs(float(ref))
    got.backward()
    assert (low.grad[1] == 0).all() and low.grad[0].abs().sum() > 0
    assert torch.equal(Fn.upsample_loss_valid_torch("l1_masked", low, lab, 4), Fn.upsample_loss_valid_torch(
        "l1_masked", low, lab, 4, torch.ones(3, dtype=torch.uint8)))


@pytest.mark.parametrize("task", TASKS)
def test_no_labelled_sample_is_exactly_zero(gold, task):
    from mtlora_amd import functional as Fn
    from mtlora_amd.mtl_harness import MultiTaskLoss, task_loss
    kind, pw = KIND[task]
    valid = torch.zeros(3, dtype=torch.uint8)
    out = gold["out"][task].float().requires_grad_(True)
    lab = torch.full_like(gold["lab"][task].float(), float("nan"))
    got = task_loss(task, out, lab, valid)
    got.backward()
    assert got.item() == 0.0 and not torch.signbit(got).item()
    assert out.grad is not None and (out.grad == 0).all()
    low = gold["out"][task].double().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    got = Fn.upsample_loss_valid_torch(kind, low, lab.double(), 1, valid, pos_weight=pw)
    got.backward()
    assert got.item() == 0.0 and not torch.signbit(got).item() and (low.grad == 0).all()
    # through the criterion, CPU plain path of task_low included
    crit = MultiTaskLoss([task])
    total, per = crit.forward({task: out}, {task: lab}, {task: valid})
    assert total.item() == 0.0 and per[task].item() == 0.0
    lo = gold["out"][task].float().permute(0, 2, 3, 1).contiguous()
    assert crit.forward_low({task: lo}, {task: lab}, {task: valid})[0].item() == 0.0


def test_multitask_loss_valid_mixes_masks_per_task(gold):
    from mtlora_amd.mtl_harness import MultiTaskLoss, task_loss
    tasks = ["semseg", "depth", "edge"]
    crit = MultiTaskLoss(tasks)
    out = {t: gold["out"][t].float() for t in tasks}
    lab = {t: gold["lab"][t].float() for t in tasks}
    valid = {"semseg": torch.tensor([1, 0, 1], dtype=torch.uint8), "depth": torch.tensor([0, 0, 1], dtype=torch.uint8)}
    total, per = crit(out, lab, valid)
    assert torch.equal(per["semseg"], task_loss("semseg", out["semseg"][[0, 2]], lab["semseg"][[0, 2]]))
    assert torch.equal(per["depth"], task_loss("depth", out["depth"][[2]], lab["depth"][[2]]))
    assert torch.equal(per["edge"], task_loss("edge", out["edge"], lab["edge"]))  # no entry: labelled everywhere
    want = sum(crit.loss_weights[t] * per[t] for t in tasks)
    assert abs(total.item() - want.item()) <= 1e-6 * abs(want.item())
    # without flags nothing moved
    t0, p0 = crit(out, lab)
    assert torch.equal(p0["semseg"], task_loss("semseg", out["semseg"], lab["semseg"]))
    low = {t: out[t].permute(0, 2, 3, 1).contiguous() for t in tasks}
    t1, p1 = crit.forward_low(low, lab, valid)  # CPU: the plain path, selection before the upsample
    for t in tasks:
        assert abs(p1[t].item() - per[t].item()) <= 1e-6 * abs(per[t].item()), t


def test_synthetic_batch_valid_poisons_the_unlabelled_labels():
    from mtlora_amd.mtl_harness import synthetic_batch
    tasks = ["semseg", "normals", "sal", "depth"]
    img0, tg0 = synthetic_batch(3, 16, tasks, seed=5)
    valid = {"semseg": [1, 0, 1], "depth": [0, 0, 0]}
    img, tg, fl = synthetic_batch(3, 16, tasks, seed=5, valid=valid)
    assert torch.equal(img, img0) and set(fl) == {"semseg", "depth"}
    assert fl["semseg"].dtype == torch.uint8 and fl["semseg"].tolist() == [1, 0, 1] and fl["depth"].tolist() == [0, 0, 0]
    assert torch.isnan(tg["semseg"][1]).all() and torch.equal(tg["semseg"][[0, 2]], tg0["semseg"][[0, 2]])
    assert torch.isnan(tg["depth"]).all()
    assert torch.equal(tg["normals"], tg0["normals"]) and torch.equal(tg["sal"], tg0["sal"])


# ------------------------------------------------------------------------------------------------
# wire batches
# ------------------------------------------------------------------------------------------------
def test_check_wire_batch_validates_the_flags():
    from mtlora_amd import data as D
    tasks = ["semseg", "depth"]
    b = D.synthetic_wire_batch(3, 8, tasks, seed=1, valid={"depth": [1, 0, 1]})
    assert D.check_wire_batch(b, tasks) == (3, 8, 8)
    assert b["valid"]["depth"].dtype == torch.uint8 and b["valid"]["depth"].tolist() == [1, 0, 1]
    assert torch.isnan(b["depth"][1]).all() and not torch.isnan(b["depth"][[0, 2]]).any()
    ref = D.synthetic_wire_batch(3, 8, tasks, seed=1)
    assert torch.equal(b["semseg"], ref["semseg"]) and torch.equal(b["depth"][[0, 2]], ref["depth"][[0, 2]])
    for bad, msg in (({"depth": torch.ones(3)}, "uint8"), ({"depth": torch.ones(2, dtype=torch.uint8)}, "uint8"),
                     ({"sal": torch.ones(3, dtype=torch.uint8)}, "not one of the tasks"), ([1, 0, 1], "dict")):
        with pytest.raises(ValueError, match=msg):
            D.check_wire_batch(dict(ref, valid=bad), tasks)
    # a task is still required to be present: the flags do not excuse a missing plane
    with pytest.raises(ValueError, match="missing"):
        D.check_wire_batch({k: v for k, v in b.items() if k != "depth"}, tasks)


def test_prepare_batch_torch_returns_the_flags_only_when_present():
    from mtlora_amd import data as D
    tasks = ["semseg", "normals", "depth"]
    plain = D.synthetic_wire_batch(3, 8, tasks, seed=2)
    assert len(D.prepare_batch_torch(plain, tasks)) == 2
    b = D.synthetic_wire_batch(3, 8, tasks, seed=2, valid={"normals": [0, 1, 1], "depth": [1, 1, 0]})
    out = D.prepare_batch_torch(b, tasks)
    assert len(out) == 3
    images, targets, valid = out
    i0, t0 = D.prepare_batch_torch(plain, tasks)
    assert torch.equal(images, i0) and torch.equal(targets["semseg"], t0["semseg"])
    assert set(valid) == {"normals", "depth"} and valid["normals"].tolist() == [0, 1, 1] and valid["depth"].dtype == torch.uint8
    assert torch.equal(targets["normals"][1:], t0["normals"][1:]) and torch.equal(targets["depth"][:2], t0["depth"][:2])


def test_merge_wire_batches_pascal_plus_nyud():
    from mtlora_amd import data as D
    from mtlora_amd.mtl_harness import NYUD4, NYUD_NUM_OUTPUT
    pascal = ["semseg", "human_parts", "sal", "normals", "edge"]
    a = D.synthetic_wire_batch(2, 8, pascal, seed=3)
    b = D.synthetic_wire_batch(1, 8, list(NYUD4), seed=4, num_outputs=NYUD_NUM_OUTPUT)
    b["flip"] = torch.tensor([1], dtype=torch.uint8)
    m, tasks = D.merge_wire_batches(a, pascal, b, NYUD4)
    assert tasks == pascal + ["depth"]
    assert D.check_wire_batch(m, tasks) == (3, 8, 8)
    want = {"semseg": [1, 1, 1], "human_parts": [1, 1, 0], "sal": [1, 1, 0], "normals": [1, 1, 1], "edge": [1, 1, 1], "depth": [0, 0, 1]}
    assert {t: v.tolist() for t, v in m["valid"].items()} == want
    assert m["flip"].tolist() == [0, 0, 1]
    assert torch.equal(m["image"], torch.cat([a["image"], b["image"]]))
    for t in tasks:
        if t in pascal:
            assert torch.equal(m[t][:2], a[t]), t
        if t in NYUD4:
            assert torch.equal(m[t][2:], b[t]), t
        assert m[t].dtype == (a[t] if t in pascal else b[t]).dtype
    images, targets, valid = D.prepare_batch_torch(m, tasks)
    ia, ta = D.prepare_batch_torch(a, pascal)
    ib, tb = D.prepare_batch_torch(b, list(NYUD4))
    assert torch.equal(images, torch.cat([ia, ib]))
    for t in tasks:  # labelled samples: what each dataset's own ingest gives
        if t in pascal:
            assert torch.equal(targets[t][:2], ta[t]), t
        if t in NYUD4:
            assert torch.equal(targets[t][2:], tb[t]), t
    assert {t: v.tolist() for t, v in valid.items()} == want
    with pytest.raises(ValueError, match="sizes differ"):
        D.merge_wire_batches(a, pascal, D.synthetic_wire_batch(1, 4, list(NYUD4), seed=4), NYUD4)
    # flags that a side already carries are kept
    a2 = dict(a, valid={"sal": torch.tensor([0, 1], dtype=torch.uint8)})
    m2, _ = D.merge_wire_batches(a2, pascal, b, NYUD4)
    assert m2["valid"]["sal"].tolist() == [0, 1, 0]


# ------------------------------------------------------------------------------------------------
# library surface
# ------------------------------------------------------------------------------------------------
NEW = ("mtlora_label_stat_valid_scratch_bytes", "mtlora_label_stat_valid", "mtlora_upsample_loss_valid")


def test_header_declares_the_new_entries():
    from mtlora_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    assert re.search(r"#define\s+MTLORA_ABI_VERSION\s+12\b", hdr) and _lib.ABI_VERSION == 12  # additive: the number stays
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    for name in NEW:
        assert name in protos and name in _lib.EXPORTS, name
        assert len(protos[name].split(",")) == len(_lib._SIGS[name][1]), name
    names = [p.split()[-1].lstrip("*") for p in protos["mtlora_label_stat_valid"].split(",")]
    assert names == ["label", "valid", "B", "n_per_sample", "kind", "ignore_index", "out", "scratch", "scratch_bytes", "stream"]
    names = [p.split()[-1].lstrip("*") for p in protos["mtlora_upsample_loss_valid"].split(",")]
    assert names == ["kind", "low", "label", "valid", "stat", "dlow", "partials", "B", "h", "w", "C", "scale", "dtype", "ignore_index",
                     "stream"]
    # the existing entries keep their signatures
    assert len(protos["mtlora_upsample_loss"].split(",")) == 14 and len(protos["mtlora_label_stat"].split(",")) == 8


def test_host_rejects_of_the_new_entries(built_lib):
    """every defect is refused on the host, before any launch (no GPU here), with the code the header states"""
    from mtlora_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    code = {n: int(re.search(r"MTLORA_" + n + r"\s*=\s*(-?\d+)", hdr).group(1))
            for n in ("ERR_NULL", "ERR_SHAPE", "ERR_ALIGN", "ERR_WORKSPACE", "ERR_UNSUPPORTED", "ERR_DTYPE")}
    P = ctypes.c_void_p
    A, MIS = 0x10000, 0x10004  # fake addresses: nothing is dereferenced on the host
    sb = L.mtlora_label_stat_valid_scratch_bytes(3, 1000)
    assert sb == 3 * 1 * 4 + 256
    assert L.mtlora_label_stat_valid_scratch_bytes(32, 448 * 448) == 32 * 25 * 4 + 256
    assert L.mtlora_label_stat_valid_scratch_bytes(0, 10) == -1 and L.mtlora_label_stat_valid_scratch_bytes(3, 0) == -1
    assert L.mtlora_label_stat_valid_scratch_bytes(3, 1 << 31) == -1 and L.mtlora_label_stat_valid_scratch_bytes(1 << 21, 4) == -1

    def stat(label=A, valid=A, B=3, n=1000, kind=0, out=A, scratch=A, sbytes=sb):
        return L.mtlora_label_stat_valid(P(label), P(valid), B, n, kind, 255.0, P(out), P(scratch), sbytes, None)

    assert stat(kind=3) == code["ERR_UNSUPPORTED"] and stat(kind=-1) == code["ERR_UNSUPPORTED"]
    assert stat(B=0) == code["ERR_SHAPE"] and stat(n=0) == code["ERR_SHAPE"] and stat(B=-1) == code["ERR_SHAPE"]
    assert stat(label=0) == code["ERR_NULL"] and stat(out=0) == code["ERR_NULL"] and stat(scratch=0) == code["ERR_NULL"]
    assert stat(label=MIS) == code["ERR_ALIGN"] and stat(scratch=MIS) == code["ERR_ALIGN"] and stat(out=A + 2) == code["ERR_ALIGN"]
    assert stat(sbytes=sb - 1) == code["ERR_WORKSPACE"]

    def loss(kind=0, low=A, label=A, valid=A, st=A, dlow=A, part=A, B=3, h=5, w=9, C=21, scale=8, dtype=_lib.F32):
        return L.mtlora_upsample_loss_valid(kind, P(low), P(label), P(valid), P(st), P(dlow), P(part), B, h, w, C, scale, dtype, 255.0,
                                            None)

    for k in ("low", "label", "valid", "st", "dlow", "part"):
        assert loss(**{k: 0}) == code["ERR_NULL"], k
    assert loss(h=0) == code["ERR_SHAPE"] and loss(C=0) == code["ERR_SHAPE"] and loss(B=-1) == code["ERR_SHAPE"]
    assert loss(B=0, valid=0) == 0  # no work: OK without a launch, like mtlora_upsample_loss
    assert loss(dtype=_lib.F16) == code["ERR_DTYPE"]
    assert loss(scale=33) == code["ERR_UNSUPPORTED"] and loss(kind=7) == code["ERR_UNSUPPORTED"]
    assert loss(kind=2, C=3) == code["ERR_UNSUPPORTED"] and loss(kind=0, C=49) == code["ERR_UNSUPPORTED"]
    assert L.mtlora_prof_kind_name(23).decode() == "k_label_stat_valid"
