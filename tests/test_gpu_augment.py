"""GPU tests of the device-side ScaleNRotate + FixedResize (csrc/augment.hip, mtlora_amd/data.py).  The reference is
``data.augment_batch_torch`` evaluated on the CPU -- itself anchored to cv2's documented conventions by tests/test_cpu_augment.py.
All coordinate arithmetic is integer on both sides, so every uint8 output, depth's sampling and the normals up to and including
the in-plane rotation must be EQUAL.  The renormalised normals and the divided depth are equal as well as long as fp32 division
and square root are correctly rounded on the device (``FLOAT_ULPS`` = 0 states that they are; the figure is printed before it
is asserted).

1. all six task kinds in one call, B in {1, 3}, canvas 40 x 48, sample sizes from (1, 1) to the full canvas, output sizes (1, 1),
   (7, 5), (16, 16), (33, 67) -- widths that are no multiple of the 16-byte store, more than one 1024-pixel block per sample --
   and every pair of rot in {0, 90, 180, -20, 17.3} and sc in {0.25, 0.75, 1, 1.25, 4}, over a sentinel-filled canvas.
2. the sentinel: another fill outside the rectangles changes no output bit.
3. sources at byte offsets 1, 2, 3; two calls; inputs untouched; the 8-job limit.
4. DeviceLoader with ``augment`` / ``out_size``: seeded epochs, ``last_geoms``, host overrides, the unchanged plain path, and
   its batches through train_step / validate_step.
"""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

ALL_TASKS = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]
HC, WC = 40, 48
SIZES = [(1, 1), (1, 48), (40, 1), (3, 5), (37, 40), (40, 48)]
PAIRS = list(itertools.product([0.0, 90.0, 180.0, -20.0, 17.3], [0.25, 0.75, 1.0, 1.25, 4.0]))
FLOAT_ULPS = 0  # division and sqrt are IEEE on the device (hipcc's default for HIP); 4 would be the allowance if they were not


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def to_dev(batch):
    return {k: v.to(dev()) for k, v in batch.items()}


@functools.lru_cache(maxsize=None)
def raw_case(sizes, seed=0):
    """a sentinel-filled canvas batch with the given sample sizes (computed once, never modified)"""
    from mtlora_amd import data as D
    raw = D.synthetic_raw_batch(len(sizes), HC, WC, ALL_TASKS, seed=seed + 17 * len(sizes), sizes=[list(s) for s in sizes])
    raw["normals"][:, 0, 0] = 0.0  # (an all-zero normal inside every rectangle)
    return raw


def ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place (+0 and -0 coincide)"""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def check(raw, geom, out_size, what=""):
    """augment_batch on the device against augment_batch_torch on the CPU, both stages of the normals"""
    from mtlora_amd import data as D
    on_dev = to_dev(raw)
    got = D.augment_batch(on_dev, ALL_TASKS, geom, out_size)
    want = D.augment_batch_torch(raw, ALL_TASKS, geom, out_size)
    assert list(got) == list(want)
    worst = 0
    for k in ["image"] + ALL_TASKS:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and got[k].is_contiguous(), f"{what} {k}"
        if k in ("normals", "depth"):
            worst = max(worst, ulps(g, want[k]))
        else:
            assert torch.equal(g, want[k]), f"{what} {k}"
    stage = D.augment_batch(on_dev, ["normals"], geom, out_size, renormalize=False)["normals"].cpu()
    assert torch.equal(stage, D.augment_batch_torch(raw, ["normals"], geom, out_size, renormalize=False)["normals"]), f"{what} normals before renorm"
    return worst


@pytest.mark.parametrize("out_size", [(1, 1), (7, 5), (16, 16), (33, 67)])
@pytest.mark.parametrize("B", [1, 3])
def test_all_kinds_sizes_rotations_scales(B, out_size):
    from mtlora_amd import data as D
    groups = [(s,) for s in SIZES] if B == 1 else [tuple(SIZES[:3]), tuple(SIZES[3:])]
    pairs = itertools.cycle(PAIRS)
    worst, n_calls = 0, 25 if B == 1 else 9  # 25 or 27 (rot, sc) pairs: every pair at least once per output size
    nonzero = 0
    for n in range(n_calls):
        raw = raw_case(groups[n % len(groups)])
        rs = [next(pairs) for _ in range(B)]
        geom = D.make_geometry(raw["size"], [r for r, _ in rs], [s for _, s in rs], out_size)
        worst = max(worst, check(raw, geom, out_size, f"sizes {groups[n % len(groups)]} rot/sc {rs}"))
    print(f"B={B} out_size={out_size}: max ulp distance of renormalised normals / divided depth = {worst}")
    assert worst <= FLOAT_ULPS, worst


def test_outputs_hold_what_the_cases_are_there_for():
    """the comparison above is not between two empty results: inside, border and all-zero-normal pixels all occur"""
    from mtlora_amd import data as D
    raw = raw_case((SIZES[4],))
    geom = D.make_geometry(raw["size"], 17.3, 0.75, (33, 67))
    got = D.augment_batch(to_dev(raw), ALL_TASKS, geom, (33, 67))
    img, sem, nrm, dep = got["image"].cpu(), got["semseg"].cpu(), got["normals"].cpu(), got["depth"].cpu()
    assert 0.3 < float((dep > 0).float().mean()) < 0.9 and bool((dep[0, 0, 0] == 0).all())   # sc < 1: a border around the sample
    assert bool((img[0, 0, 0] == 0).all()) and int(img.max()) > 200
    assert not bool((sem == 200).any()) and float(dep.max()) < 10 / 0.75 + 1e-3 and float(nrm.abs().max()) <= 1.0  # no sentinel
    inside = (nrm != 0).any(-1)
    assert float((nrm[inside].double().norm(dim=-1) - 1).abs().max()) <= 4 * 2 ** -23


def test_sentinel_does_not_leak():
    """another canvas fill outside the rectangles -- edges of the rectangle and negative source coordinates included (sc 0.25
    and 4, rot -20) -- changes no output bit"""
    from mtlora_amd import data as D
    raw = raw_case(tuple(SIZES[3:]))
    other = {k: v.clone() for k, v in raw.items()}
    for b, (h, w) in enumerate(SIZES[3:]):
        for k in ["image"] + ALL_TASKS:
            other[k][b, h:] = 0
            other[k][b, :, w:] = 1
    for rot, sc in ((-20.0, 0.25), (17.3, 4.0), (0.0, 1.0)):
        geom = D.make_geometry(raw["size"], rot, sc, (33, 67))
        a, b = D.augment_batch(to_dev(raw), ALL_TASKS, geom, (33, 67)), D.augment_batch(to_dev(other), ALL_TASKS, geom, (33, 67))
        for k in ["image"] + ALL_TASKS:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (k, rot, sc)


def _offset_copy(t, off):
    """``t`` on the device, as a contiguous slice starting ``off`` elements into a larger buffer filled with a poison value"""
    poison = 0xA5 if t.dtype == torch.uint8 else float("nan")
    buf = torch.full((t.numel() + off + 7,), poison, dtype=t.dtype, device=dev())
    buf[off:off + t.numel()] = t.to(dev()).flatten()
    return buf, buf[off:off + t.numel()].view(t.shape)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_source_alignment(off):
    """uint8 sources at byte offsets 1, 2, 3; fp32 sources one element in (4 bytes off a 16-byte line)"""
    from mtlora_amd import data as D
    raw = raw_case(tuple(SIZES[3:]))
    geom = D.make_geometry(raw["size"], [17.3, -20.0, 90.0], [1.25, 0.75, 1.0], (33, 67))
    want = D.augment_batch_torch(raw, ALL_TASKS, geom, (33, 67))
    batch, bufs = {"size": raw["size"].to(dev())}, {}
    for k in ["image"] + ALL_TASKS:
        bufs[k], batch[k] = _offset_copy(raw[k], off if raw[k].dtype == torch.uint8 else 1)
        assert batch[k].data_ptr() % 16 != 0 and batch[k].is_contiguous()
    before = {k: v.clone() for k, v in bufs.items()}
    got = D.augment_batch(batch, ALL_TASKS, geom, (33, 67))
    for k in ["image"] + ALL_TASKS:
        if k in ("normals", "depth"):
            assert ulps(got[k].cpu(), want[k]) <= FLOAT_ULPS, k
        else:
            assert torch.equal(got[k].cpu(), want[k]), k
    for k in bufs:  # sources and their surroundings untouched (NaN poison: compare the bytes)
        assert torch.equal(bufs[k].view(torch.uint8), before[k].view(torch.uint8)), k


def test_two_calls_give_equal_outputs_and_inputs_stay():
    from mtlora_amd import data as D
    raw = raw_case(tuple(SIZES[3:]))
    geom = D.make_geometry(raw["size"], [17.3, -20.0, 180.0], [0.75, 1.25, 4.0], (33, 67))
    batch = to_dev(raw)
    before = {k: v.clone() for k, v in batch.items()}
    dgeom = D.Geometry(geom.coef.to(dev()), geom.side.to(dev()))  # (a geometry already on the device is taken as it is)
    a, b = D.augment_batch(batch, ALL_TASKS, geom, (33, 67)), D.augment_batch(batch, ALL_TASKS, dgeom, (33, 67))
    for k in ["image"] + ALL_TASKS:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    for k in batch:
        assert torch.equal(batch[k], before[k]), k
    assert D.check_wire_batch(a, ALL_TASKS) == (3, 33, 67)
    # the result goes straight into the ingest, flags passing through
    flip = torch.tensor([1, 0, 1], dtype=torch.uint8)
    wire = D.augment_batch({**batch, "flip": flip.to(dev())}, ALL_TASKS, geom, (33, 67))
    img, tg = D.prepare_batch(wire, ALL_TASKS)
    ref_img, ref_tg = D.prepare_batch_torch({**{k: v.cpu() for k, v in a.items()}, "flip": flip}, ALL_TASKS)
    assert torch.equal(img.cpu(), ref_img) and all(torch.equal(tg[t].cpu(), ref_tg[t]) for t in ALL_TASKS)


def test_eight_job_limit():
    from mtlora_amd import data as D
    from mtlora_amd import functional as Fn
    raw = raw_case(tuple(SIZES[3:]))
    geom = D.make_geometry(raw["size"], 17.3, 1.25, (7, 5))
    seven = ALL_TASKS + ["t0"]  # image + 7 tasks = 8 jobs (t0: a synthetic task in the normals format)
    batch = to_dev({**raw, "t0": raw["normals"].flip(-1).contiguous(), "t1": raw["normals"]})
    got = D.augment_batch(batch, seven, geom, (7, 5))
    want = D.augment_batch_torch({k: v.cpu() for k, v in batch.items()}, seven, geom, (7, 5))
    for k in ["image"] + seven:
        if k in ("normals", "depth", "t0"):
            assert ulps(got[k].cpu(), want[k]) <= FLOAT_ULPS, k
        else:
            assert torch.equal(got[k].cpu(), want[k]), k
    with pytest.raises(RuntimeError, match="at most 7 tasks"):
        D.augment_batch(batch, seven + ["t1"], geom, (7, 5))
    q15, f32 = (t.to(dev()) for t in D.cubic_table())
    with pytest.raises(RuntimeError, match="mtlora_augment_batch failed"):   # the library's own check, through the thin wrapper
        Fn.augment_batch([("class_nearest_u8", batch["sal"])] * 9, batch["size"], geom.coef.to(dev()), geom.side.to(dev()), (7, 5), q15, f32)
    outs = Fn.augment_batch([("class_nearest_u8", batch["sal"])] * 8, batch["size"], geom.coef.to(dev()), geom.side.to(dev()), (7, 5))
    assert len(outs) == 8 and all(torch.equal(o.cpu(), want["sal"]) for o in outs)


def _cpu(out):
    return out[0].cpu(), {t: v.cpu() for t, v in out[1].items()}


def test_device_loader_augments_with_a_seed():
    """five raw batches through a ring of two, two epochs: bit-identical; last_geoms / last_flips reproduce every batch through
    the two definitions; host rot_deg / scale entries override the draw; another seed draws another epoch"""
    from mtlora_amd import data as D
    tasks = ["semseg", "human_parts", "normals", "depth"]
    host = [D.synthetic_raw_batch(3, HC, WC, tasks, seed=200 + i) for i in range(5)]
    host[3] = {**host[3], "rot_deg": [90.0, 0.0, -20.0]}
    host[4] = {**host[4], "rot_deg": torch.tensor([17.3, 0.0, 180.0]), "scale": [1.0, 4.0, 0.25]}
    aug = dict(rots=(-20, 20), scales=(.75, 1.25))
    runs = []
    for _ in range(2):
        dl = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=11, depth=2, augment=aug, out_size=(33, 67))
        runs.append(([_cpu(o) for o in dl], list(dl.last_flips), list(dl.last_geoms)))
    (got, flips, geoms), (got2, flips2, geoms2) = runs
    assert len(got) == len(flips) == len(geoms) == 5
    for i in range(5):
        assert torch.equal(flips[i], flips2[i]) and torch.equal(geoms[i].coef, geoms2[i].coef) and torch.equal(geoms[i].side, geoms2[i].side)
        wire = D.augment_batch_torch(host[i], tasks, geoms[i], (33, 67))
        if FLOAT_ULPS == 0:
            want = D.prepare_batch_torch({**wire, "flip": flips[i]}, tasks)
            for a in (got[i], got2[i]):
                assert torch.equal(a[0], want[0]) and all(torch.equal(a[1][t], want[1][t]) for t in tasks), i
        assert torch.equal(got[i][0], got2[i][0]) and all(torch.equal(got[i][1][t], got2[i][1][t]) for t in tasks), i
        assert got[i][0].shape == (3, 3, 33, 67)
    assert geoms[4].side[:, 2].tolist() == [1.0, 4.0, 0.25] and geoms[4].side[2, :2].tolist() == [-1.0, 0.0]   # host entries win
    assert geoms[3].side[0, :2].tolist() == [0.0, 1.0] and bool((geoms[3].side[:, 2] != 1).all())             # (scale still drawn)
    assert bool((geoms[0].side[:, 2] >= 0.75).all()) and bool((geoms[0].side[:, 2] <= 1.25).all())
    other = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=12, augment=aug, out_size=(33, 67))
    list(other)
    assert not torch.equal(other.last_geoms[0].coef, geoms[0].coef)
    # the draws are the documented ones: flips first, then rot, then scale, per batch, from the one generator
    gen = torch.Generator().manual_seed(11)
    fl = (torch.rand(3, generator=gen) < 0.5).to(torch.uint8)
    rot = 40.0 * torch.rand(3, generator=gen, dtype=torch.float64) - 20.0
    sc = 0.5 * torch.rand(3, generator=gen, dtype=torch.float64) - 0.25 + 1.0
    assert torch.equal(fl, flips[0]) and torch.equal(geoms[0].coef, D.make_geometry(host[0]["size"], rot, sc, (33, 67)).coef)


def test_device_loader_without_augment_is_unchanged_and_out_size_alone_resizes():
    from mtlora_amd import data as D
    tasks = ["semseg", "human_parts", "normals", "depth"]
    host = [D.synthetic_wire_batch(3, 40, tasks, seed=100 + i) for i in range(3)]
    dl = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=11, depth=2)
    got = [_cpu(o) for o in dl]
    gen = torch.Generator().manual_seed(11)
    for i in range(3):
        fl = (torch.rand(3, generator=gen) < 0.5).to(torch.uint8)   # the random stream of the plain loader: B numbers per batch
        assert torch.equal(dl.last_flips[i], fl) and dl.last_geoms[i] is None
        img, tg = D.prepare_batch({**to_dev(host[i]), "flip": fl.to(dev())}, tasks)
        assert torch.equal(got[i][0], img.cpu()) and all(torch.equal(got[i][1][t], tg[t].cpu()) for t in tasks)
    # out_size alone: the test pipeline (rot 0, sc 1), nothing drawn
    raw = [D.synthetic_raw_batch(2, HC, WC, tasks, seed=300 + i) for i in range(2)]
    rl = D.DeviceLoader(raw, tasks, dev(), out_size=(16, 16))
    out = [_cpu(o) for o in rl]
    for i in range(2):
        assert rl.last_flips[i] is None and rl.last_geoms[i].side.tolist() == [[1.0, 0.0, 1.0]] * 2
        geom = D.make_geometry(raw[i]["size"], 0.0, 1.0, (16, 16))
        assert torch.equal(rl.last_geoms[i].coef, geom.coef)
        wire = D.augment_batch(to_dev(raw[i]), tasks, geom, (16, 16))
        img, tg = D.prepare_batch(wire, tasks)
        assert torch.equal(out[i][0], img.cpu()) and all(torch.equal(out[i][1][t], tg[t].cpu()) for t in tasks)


def test_augmenting_loader_feeds_train_and_validate_step():
    """one train_step and one validate_step of the small 224 px model on what an augmenting DeviceLoader yields"""
    from mtlora_amd import data as D
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter
    tasks = ["semseg", "normals", "sal", "human_parts"]
    host = [D.synthetic_raw_batch(2, 250, 260, tasks, seed=21 + i) for i in range(2)]
    dl = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=4, augment=dict(rots=(-20, 20), scales=(.75, 1.25)), out_size=(224, 224))
    fed = list(dl)
    assert fed[0][0].shape == (2, 3, 224, 224) and fed[0][1]["normals"].shape == (2, 3, 224, 224)
    torch.manual_seed(5)
    Fn._seed_counter = 0
    Fn.droppath_reset()
    model = H.build_model(img_size=224, tasks=tasks, r_shared=16, r_task=4, seed=0).to(dev()).train()
    crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3)
    loss, _ = H.train_step(model, crit, opt, *fed[0])
    vloss, per = H.validate_step(model, crit, PerformanceMeter(tasks), *fed[1])
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(vloss) and all(bool(torch.isfinite(v).all()) for v in per.values())
