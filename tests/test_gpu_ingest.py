"""GPU tests of the batch ingest (csrc/ingest.hip, mtlora_amd/data.py).  The reference is ``data.prepare_batch_torch`` evaluated
on the CPU -- itself held to the reference's real transform classes by tests/test_cpu_ingest.py -- and every comparison is
``torch.equal``: nothing here resamples or rounds, so there is no tolerance.

1. shapes: rows shorter than one 16-byte vector, unaligned row ends on both sides (W % 4 != 0, H W % 4 != 0), flipped and
   unflipped samples in one batch, more than one row block, and the full-vector path at W = 448 (two row segments).
2. sources at odd byte / element offsets inside a larger buffer.
3. the human_parts rule: all-zero, only the last pixel set, only the first pixel set; a plain class map in the same call.
4. normals (+-0, one zero component, denormals, fp16 source, sign of channel 0 under the flip) and depth zeros, bit for bit.
5. two calls give equal outputs, inputs are untouched, nothing around the sources' slices was needed.
6. DeviceLoader: ring reuse, seeded flips, and its batches through train_step / validate_step.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ALL_TASKS = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def to_dev(batch):
    return {k: v.to(dev()) for k, v in batch.items()}


@functools.lru_cache(maxsize=None)
def case(B, H, W, normals_dtype=torch.float32):
    """a wire batch with every edge value in it, mixed flip flags, and its CPU restatement (computed once, never modified)"""
    from mtlora_amd import data as D
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
    wire = {"image": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)}
    for t, n in (("semseg", 21), ("human_parts", 7)):
        wire[t] = torch.randint(0, n, (B, H, W), generator=g, dtype=torch.uint8)
        wire[t][torch.rand(B, H, W, generator=g) < 0.1] = 255
    wire["human_parts"][0] = 0
    wire["sal"] = (torch.rand(B, H, W, generator=g) < 0.3).to(torch.uint8)
    wire["edge"] = (torch.rand(B, H, W, generator=g) < 0.1).to(torch.uint8)
    nrm = torch.nn.functional.normalize(torch.randn(B, H, W, 3, generator=g), dim=-1)
    nrm[torch.rand(B, H, W, generator=g) < 0.2] = 0.0
    nrm[..., 0][torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    wire["normals"] = nrm.to(normals_dtype)
    dep = torch.rand(B, H, W, generator=g) * 10
    dep[torch.rand(B, H, W, generator=g) < 0.2] = 0.0
    wire["depth"] = dep
    wire["flip"] = (torch.arange(B) % 2 == 0).to(torch.uint8)  # B = 1: flipped; B = 3: 1, 0, 1
    if B == 1 and H == 3:
        wire["flip"] = torch.zeros(1, dtype=torch.uint8)  # (and one unflipped single sample)
    return wire, D.prepare_batch_torch(wire, ALL_TASKS)


def check(got, want, what=""):
    img, tg = got
    assert img.dtype == torch.float32 and torch.equal(img.cpu(), want[0]), f"{what} image"
    assert list(tg) == list(want[1])
    for t in tg:
        assert tg[t].dtype == torch.float32 and tg[t].is_contiguous() and tg[t].shape == want[1][t].shape, f"{what} {t}"
        assert torch.equal(tg[t].cpu(), want[1][t]), f"{what} {t}"


@pytest.mark.parametrize("W", [1, 5, 16, 37, 67])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
def test_shapes_all_six_tasks(B, H, W):
    from mtlora_amd import data as D
    wire, want = case(B, H, W)
    check(D.prepare_batch(to_dev(wire), ALL_TASKS), want)


def test_full_vector_rows():
    """W = 448: two row segments (256 + 192 pixels), every chunk but the ends a 16-byte access"""
    from mtlora_amd import data as D
    wire, want = case(2, 8, 448)
    check(D.prepare_batch(to_dev(wire), ALL_TASKS), want)


def test_more_than_one_row_block_and_fp16_normals():
    """H = 37: three row blocks of 16 rows, the last one partial; W = 257: a second segment of one pixel"""
    from mtlora_amd import data as D
    wire, want = case(2, 37, 257, torch.float16)
    assert bool((want[1]["normals"] == 255).any())
    check(D.prepare_batch(to_dev(wire), ALL_TASKS), want)


def _offset_copy(t, off):
    """``t`` on the device, as a contiguous slice starting ``off`` elements into a larger buffer filled with a poison value"""
    poison = 0xA5 if t.dtype == torch.uint8 else float("nan")
    buf = torch.full((t.numel() + off + 7,), poison, dtype=t.dtype, device=dev())
    buf[off:off + t.numel()] = t.to(dev()).flatten()
    return buf, buf[off:off + t.numel()].view(t.shape)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_source_alignment(off):
    """uint8 sources at byte offsets 1, 2, 3; fp32 and fp16 sources one element in (4 and 2 bytes off a 16-byte line)"""
    from mtlora_amd import data as D
    for shape, nd in (((3, 3, 37), torch.float32), ((2, 8, 448), torch.float16 if off == 2 else torch.float32)):
        wire, want = case(*shape, nd)
        batch, bufs = {"flip": wire["flip"].to(dev())}, {}
        for k in ["image"] + ALL_TASKS:
            bufs[k], batch[k] = _offset_copy(wire[k], off if wire[k].dtype == torch.uint8 else 1)
            assert batch[k].data_ptr() % 16 != 0 and batch[k].is_contiguous()
        before = {k: v.clone() for k, v in bufs.items()}
        check(D.prepare_batch(batch, ALL_TASKS), want, f"offset {off}")
        for k in bufs:  # sources and their surroundings untouched (NaN poison: compare the bytes)
            assert torch.equal(bufs[k].view(torch.uint8), before[k].view(torch.uint8)), k


def test_human_parts_rule():
    from mtlora_amd import data as D
    from mtlora_amd import functional as Fn
    B, H, W = 4, 5, 37
    hp = torch.zeros(B, H, W, dtype=torch.uint8)
    hp[1, -1, -1] = 3   # only the last pixel
    hp[2, 0, 0] = 255   # only the first pixel (an ignore label is not 0)
    hp[3, 2, 17] = 1
    sem = torch.zeros(B, H, W, dtype=torch.uint8)  # a plain class map that is 0 everywhere stays 0
    sem[2] = 7
    flip = torch.tensor([1, 1, 0, 1], dtype=torch.uint8)
    wire = {"image": torch.zeros(B, H, W, 3, dtype=torch.uint8), "human_parts": hp, "semseg": sem, "flip": flip}
    tasks = ["human_parts", "semseg"]
    want = D.prepare_batch_torch(wire, tasks)
    assert bool((want[1]["human_parts"][0] == 255).all()) and want[1]["human_parts"][1].sum() == 3 and want[1]["human_parts"][1, 0, -1, 0] == 3
    assert bool((want[1]["semseg"][0] == 0).all()) and want[1]["human_parts"][2].sum() == 255
    check(D.prepare_batch(to_dev(wire), tasks), want)
    # through the thin wrapper: no image job, no flags, two jobs with the rule (each with flag words of its own) around a plain one
    hp2 = hp.flip(0).contiguous()
    outs = Fn.ingest_batch([("class_allzero_ignore", hp.to(dev())), ("class", sem.to(dev())), ("class_allzero_ignore", hp2.to(dev()))])
    ref = D.prepare_batch_torch({"image": wire["image"], "human_parts": hp, "semseg": sem}, tasks)[1]
    ref2 = D.prepare_batch_torch({"image": wire["image"], "human_parts": hp2}, ["human_parts"])[1]
    assert bool((ref2["human_parts"][3] == 255).all()) and ref2["human_parts"][0].sum() == 1
    assert torch.equal(outs[0].cpu(), ref["human_parts"]) and torch.equal(outs[1].cpu(), ref["semseg"])
    assert torch.equal(outs[2].cpu(), ref2["human_parts"])


@pytest.mark.parametrize("nd", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_normals_and_depth_edge_values(nd):
    from mtlora_amd import data as D
    sub = 1e-45 if nd == torch.float32 else 6e-8  # the smallest denormal of the source type
    px = torch.tensor([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8], [0.6, 0.8, 0.0],
                       [sub, 0.0, 0.0], [0.0, 0.0, -sub], [-1.0, 0.0, 0.0], [1.0, 0.0, -0.0], [0.0, 1.0, 0.0], [2.0, -3.0, 4.0]]).to(nd)
    B, H, W = 2, 3, 12
    nrm = px.view(1, 1, W, 3).expand(B, H, W, 3).contiguous()
    assert int((nrm[0, 0].float() != 0).any(-1).sum()) == W - 3
    dep = torch.tensor([0.0, -0.0, 1e-45, 1.0, 255.0, 0.0, 3.5, 0.0, 9.0, -1e-45, 0.0, 2.0]).view(1, 1, W).expand(B, H, W).contiguous()
    wire = {"image": torch.zeros(B, H, W, 3, dtype=torch.uint8), "normals": nrm, "depth": dep, "flip": torch.tensor([0, 1], dtype=torch.uint8)}
    want = D.prepare_batch_torch(wire, ["normals", "depth"])
    n = want[1]["normals"]
    m = n[0, 0].flip(-1)
    assert torch.equal(n[1, 0], torch.where(m == 255, m, -m))  # channel 0: mirrored and negated (ignore pixels stay 255)
    assert torch.equal(n[1, 1:], n[0, 1:].flip(-1))             # channels 1, 2: mirrored only
    got = D.prepare_batch(to_dev(wire), ["normals", "depth"])
    check(got, want)
    for t in ("normals", "depth"):  # and the bits: the sign of a zero, denormals kept
        assert torch.equal(got[1][t].cpu().view(torch.int32), want[1][t].view(torch.int32)), t


def test_two_calls_give_equal_outputs_and_inputs_stay():
    from mtlora_amd import data as D
    wire, want = case(3, 3, 67)
    batch = to_dev(wire)
    before = {k: v.clone() for k, v in batch.items()}
    a = D.prepare_batch(batch, ALL_TASKS)
    b = D.prepare_batch(batch, ALL_TASKS)
    check(a, want)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][t], b[1][t]) for t in ALL_TASKS)
    for k in batch:
        assert torch.equal(batch[k], before[k]), k
    # explicit flags override the batch's; none at all: the test pipeline
    flipped = D.prepare_batch(batch, ALL_TASKS, flip=1 - batch["flip"])
    check(flipped, D.prepare_batch_torch({**wire, "flip": 1 - wire["flip"]}, ALL_TASKS), "inverted flags")
    plain = {k: v for k, v in batch.items() if k != "flip"}
    check(D.prepare_batch(plain, ALL_TASKS), D.prepare_batch_torch({k: v for k, v in wire.items() if k != "flip"}, ALL_TASKS), "no flags")


def test_device_loader_ring_and_seed():
    """five batches through a ring of two: batch k + 1 is requested (its staging filled, batch k + 2 submitted into batch k's
    slot) before batch k is looked at, so a ring slot reused too early -- or an output living in the ring -- would show"""
    from mtlora_amd import data as D
    tasks = ["semseg", "human_parts", "normals", "depth"]
    host = [D.synthetic_wire_batch(3, 40, tasks, seed=100 + i) for i in range(5)]
    runs = []
    for _ in range(2):
        dl = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=11, depth=2)
        it = iter(dl)
        got, prev = [], next(it)
        for nxt in it:
            got.append((prev[0].cpu(), {t: v.cpu() for t, v in prev[1].items()}))
            prev = nxt
        got.append((prev[0].cpu(), {t: v.cpu() for t, v in prev[1].items()}))
        runs.append((got, [f.clone() for f in dl.last_flips]))
    (got, flips), (got2, flips2) = runs
    assert len(got) == 5 and len(flips) == 5
    assert all(torch.equal(a, b) for a, b in zip(flips, flips2))          # the seed reproduces the epoch's flips
    assert 0 < sum(int(f.sum()) for f in flips) < 15                       # (both states occur)
    for i in range(5):
        want = D.prepare_batch_torch({**host[i], "flip": flips[i]}, tasks)
        check(got[i], want, f"batch {i}")
        check(got2[i], want, f"second epoch, batch {i}")
    other = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=12, depth=2)
    list(other)
    assert any(not torch.equal(a, b) for a, b in zip(flips, other.last_flips))
    # depth 1 and a ring deeper than the epoch; no flips by default
    for depth in (1, 7):
        out = list(D.DeviceLoader(host[:2], tasks, dev(), depth=depth))
        for i in range(2):
            check(out[i], D.prepare_batch_torch(host[i], tasks), f"depth {depth}")


def test_device_loader_feeds_train_and_validate_step():
    """one train_step and one validate_step of the small 224 px model on what DeviceLoader yields: the losses are those of the
    same steps on the CPU restatement's tensors moved to the device (same seeds, bit-identical inputs, deterministic kernels)"""
    from mtlora_amd import data as D
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter
    tasks = ["semseg", "normals", "sal", "human_parts"]
    host = [D.synthetic_wire_batch(2, 224, tasks, seed=21 + i) for i in range(2)]
    dl = D.DeviceLoader(host, tasks, dev(), flip_p=0.5, seed=4)
    fed = list(dl)
    plain = []
    for i in range(2):
        img, tg = D.prepare_batch_torch({**host[i], "flip": dl.last_flips[i]}, tasks)
        plain.append((img.to(dev()), {t: v.to(dev()) for t, v in tg.items()}))
    results = []
    for batches in (fed, plain):
        torch.manual_seed(5)
        Fn._seed_counter = 0
        Fn.droppath_reset()
        model = H.build_model(img_size=224, tasks=tasks, r_shared=16, r_task=4, seed=0).to(dev()).train()
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3)
        loss, _ = H.train_step(model, crit, opt, *batches[0])
        vloss, per = H.validate_step(model, crit, PerformanceMeter(tasks), *batches[1])
        torch.cuda.synchronize()
        results.append((loss.clone(), vloss.clone(), {t: v.clone() for t, v in per.items()}))
    (l0, v0, p0), (l1, v1, p1) = results
    assert torch.isfinite(l0) and torch.isfinite(v0)
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    assert torch.equal(v0, v1), (v0.item(), v1.item())
    for t in tasks:
        assert torch.equal(p0[t], p1[t]), t
