"""CPU tests of the batch ingest (csrc/ingest.hip through the C ABI, mtlora_amd/data.py): the torch restatement against the
tensors the reference's real transform classes returned (tests/golden/ingest_tail.pt, made by make_golden_ingest.py), the
all-zero normals rule against the reference's formula in float64, every rejection of the library before a launch, the header
against the ctypes binding, DeviceLoader's argument checks and the synthetic wire batch.  No GPU needed: every library call
here returns before it touches a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TASKS = ["semseg", "human_parts", "sal", "edge", "normals", "depth"]


@pytest.fixture(scope="module")
def lib():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    return _lib.lib()


def test_restatement_equals_the_reference_classes(golden):
    """RandomHorizontalFlip -> AddIgnoreRegions -> ToTensor -> Normalize of the reference, bit for bit, every sample in both
    flip states; the wire inputs are not modified"""
    from mtlora_amd import data as D
    rec = golden("ingest_tail.pt")
    assert rec["tasks"] == ALL_TASKS and sorted(map(tuple, rec["flips"])) == [(0, 1), (1, 0)]
    before = {k: v.clone() for k, v in rec["wire"].items()}
    for pattern, want in zip(rec["flips"], rec["outputs"]):
        batch = dict(rec["wire"], flip=torch.tensor(pattern, dtype=torch.uint8))
        img, tg = D.prepare_batch_torch(batch, rec["tasks"], rec["mean"], rec["std"])
        assert img.dtype == torch.float32 and torch.equal(img, want["image"])
        for t in rec["tasks"]:
            assert tg[t].dtype == torch.float32 and tg[t].is_contiguous() and torch.equal(tg[t], want[t]), (pattern, t)
    # the fixture holds the cases it is there for
    assert bool((rec["wire"]["human_parts"][0] == 0).all()) and bool((rec["outputs"][0]["human_parts"][0] == 255).all())
    assert bool((rec["outputs"][0]["normals"] == 255).any()) and bool((rec["outputs"][0]["depth"] == 255).any())
    for k, v in before.items():
        assert torch.equal(rec["wire"][k], v), k
    # without flags: the test pipeline (no RandomHorizontalFlip); flip [0, 1] has sample 0 unflipped, [1, 0] sample 1
    img, tg = D.prepare_batch_torch(rec["wire"], rec["tasks"])
    for b, o in ((0, rec["outputs"][rec["flips"].index([0, 1])]), (1, rec["outputs"][rec["flips"].index([1, 0])])):
        assert torch.equal(img[b], o["image"][b])
        for t in rec["tasks"]:
            assert torch.equal(tg[t][b], o[t][b]), t


def test_image_table_is_what_the_two_transforms_compute():
    from mtlora_amd import data as D
    lut = D.image_table()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous()  # a (1, 256, 1, 3) image
    img, _ = D.prepare_batch_torch({"image": u8}, [])
    assert torch.equal(img[0, :, :, 0], lut)


def test_allzero_normals_rule_is_the_float64_formula():
    """AddIgnoreRegions: Nn = sqrt(x^2 + y^2 + z^2) in float64, pixels with Nn == 0 become 255 -- against "all three are 0" of
    the restatement, on fp32 inputs with denormals, -0.0, the largest and smallest normals, and fp16 inputs"""
    from mtlora_amd import data as D
    tiny, sub = float(np.finfo(np.float32).tiny), float(np.float32(1e-45))
    vals = [0.0, -0.0, sub, -sub, tiny, -tiny, 1e-30, 1.0, -1.0, float(np.finfo(np.float32).max)]
    px = torch.tensor([[a, b, c] for a in vals for b in vals for c in vals], dtype=torch.float32)  # every triple
    n = px.shape[0]
    for dtype in (torch.float32, torch.float16):
        src = px.to(dtype)
        if dtype == torch.float16:
            assert bool((src[(px == sub).any(1)] == 0).any())  # (fp16 flushes what it cannot hold: the rule sees the stored value)
        batch = {"image": torch.zeros(1, 1, n, 3, dtype=torch.uint8), "normals": src.view(1, 1, n, 3)}
        _, tg = D.prepare_batch_torch(batch, ["normals"])
        got = tg["normals"][0, :, 0, :].t()  # (n, 3)
        ref = src.double().numpy().copy()
        with np.errstate(over="ignore"):
            nn = np.sqrt(ref[:, 0] ** 2 + ref[:, 1] ** 2 + ref[:, 2] ** 2)
        ref[nn == 0, :] = 255.0
        assert 0 < int((nn == 0).sum()) < n
        assert np.array_equal(got.double().numpy(), ref)


def _job(L, kind, dtype, C, src=1 << 20, dst=1 << 21):
    j = L.IngestJob()
    j.src, j.dst, j.kind, j.src_dtype, j.C = src, dst, kind, dtype, C
    return j


def _call(lib, jobs, n_jobs=None, B=2, H=4, W=5, lut=1 << 22, scratch=1 << 23, scratch_bytes=1 << 10):
    from mtlora_amd import _lib as L
    arr = (L.IngestJob * 9)(*jobs)
    return lib.mtlora_ingest_batch(arr, len(jobs) if n_jobs is None else n_jobs, B, H, W, None, lut, scratch, scratch_bytes, None)


def test_rejections_happen_before_any_launch(lib):
    """the pointers are made-up addresses: a call that got past the checks would launch on them.  Every call here must come
    back with its status instead."""
    from mtlora_amd import _lib as L
    UNSUPPORTED, DTYPE = -7, -1
    img, cls, hp = _job(L, L.INGEST_IMAGE, L.U8, 3), _job(L, L.INGEST_CLASS, L.U8, 1), _job(L, L.INGEST_CLASS_ALLZERO_IGNORE, L.U8, 1)
    nrm, dep = _job(L, L.INGEST_NORMALS, L.F32, 3), _job(L, L.INGEST_DEPTH, L.F32, 1)
    assert _call(lib, [], n_jobs=0) == UNSUPPORTED                                   # n_jobs outside 1..8
    assert _call(lib, [cls] * 9) == UNSUPPORTED
    assert _call(lib, [cls], n_jobs=-1) == UNSUPPORTED
    assert lib.mtlora_ingest_batch(None, 1, 2, 4, 5, None, None, None, 0, None) == UNSUPPORTED
    assert _call(lib, [_job(L, 5, L.U8, 1)]) == UNSUPPORTED                          # unknown kinds
    assert _call(lib, [_job(L, -1, L.U8, 1)]) == UNSUPPORTED
    for kind, bad in ((L.INGEST_IMAGE, (L.F32, L.F16, L.BF16)), (L.INGEST_CLASS, (L.F32, L.F16)),
                      (L.INGEST_CLASS_ALLZERO_IGNORE, (L.F32,)), (L.INGEST_NORMALS, (L.U8, L.BF16, 9)),
                      (L.INGEST_DEPTH, (L.U8, L.F16, L.BF16))):
        for dt in bad:                                                               # wrong src_dtype for the kind
            assert _call(lib, [_job(L, kind, dt, 3 if kind in (L.INGEST_IMAGE, L.INGEST_NORMALS) else 1)]) == DTYPE, (kind, dt)
    for kind, dt, bad_c in ((L.INGEST_IMAGE, L.U8, (1, 4)), (L.INGEST_CLASS, L.U8, (3, 0)), (L.INGEST_CLASS_ALLZERO_IGNORE, L.U8, (3,)),
                            (L.INGEST_NORMALS, L.F32, (1, 4)), (L.INGEST_NORMALS, L.F16, (1,)), (L.INGEST_DEPTH, L.F32, (3,))):
        for C in bad_c:                                                              # C not what the kind takes
            assert _call(lib, [_job(L, kind, dt, C)]) == UNSUPPORTED, (kind, C)
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-3)):             # H, W or B < 1
        assert _call(lib, [cls, nrm], **kw) == UNSUPPORTED, kw
    assert _call(lib, [_job(L, L.INGEST_CLASS, L.U8, 1, src=0)]) == UNSUPPORTED      # null pointers
    assert _call(lib, [_job(L, L.INGEST_DEPTH, L.F32, 1, dst=0)]) == UNSUPPORTED
    assert _call(lib, [cls, _job(L, L.INGEST_NORMALS, L.F16, 3, src=0)]) == UNSUPPORTED  # (in a later job of the list)
    assert _call(lib, [img], lut=None) == UNSUPPORTED                                # an IMAGE job without a table
    assert _call(lib, [cls, dep, img], lut=None) == UNSUPPORTED
    # beyond the issue's list: what would make the kernel's vector accesses misaligned or its flags overflow
    assert _call(lib, [_job(L, L.INGEST_DEPTH, L.F32, 1, src=(1 << 20) + 2)]) == -3
    assert _call(lib, [_job(L, L.INGEST_NORMALS, L.F16, 3, src=(1 << 20) + 1)]) == -3
    assert _call(lib, [_job(L, L.INGEST_CLASS, L.U8, 1, dst=(1 << 21) + 1)]) == -3
    assert _call(lib, [hp], scratch=None) == -5 and _call(lib, [cls, hp], scratch_bytes=12) == -5
    assert lib.mtlora_ingest_scratch_bytes(2, 2) == 16 and lib.mtlora_ingest_scratch_bytes(8, 32) == 1024
    assert lib.mtlora_ingest_scratch_bytes(0, 2) < 0 and lib.mtlora_ingest_scratch_bytes(9, 2) < 0 and lib.mtlora_ingest_scratch_bytes(1, 0) < 0


def test_header_prototypes_match_ctypes(lib):
    from mtlora_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    assert "#define MTLORA_ABI_VERSION 12" in hdr and L.ABI_VERSION == 12 == lib.mtlora_version()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name in ("mtlora_ingest_scratch_bytes", "mtlora_ingest_batch"):
        assert name in L.EXPORTS
        res, args = L._SIGS[name]
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or a is ctypes.POINTER(L.IngestJob), (name, p)
                assert (a is ctypes.POINTER(L.IngestJob)) == ("mtlora_ingest_job" in p), (name, p)
            else:
                assert a is ctype_of[p.split()[0]], (name, p)
        ret = re.search(r"(\w+)\s+" + name + r"\s*\(", hdr).group(1)
        assert res is ctype_of[ret], name
    # the job struct as the header lays it out: two pointers and four int32
    m = re.search(r"typedef struct mtlora_ingest_job \{(.*?)\} mtlora_ingest_job;", hdr, flags=re.S)
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["const void* src", "void* dst", "int32_t kind, src_dtype, C, reserved"]
    assert [f[0] for f in L.IngestJob._fields_] == ["src", "dst", "kind", "src_dtype", "C", "reserved"]
    assert ctypes.sizeof(L.IngestJob) == 32 and L.IngestJob.kind.offset == 16 and L.IngestJob.C.offset == 24
    kinds = dict(re.findall(r"MTLORA_INGEST_([A-Z_]+) = (\d)", hdr))
    assert {k: int(v) for k, v in kinds.items()} == {"IMAGE": L.INGEST_IMAGE, "CLASS": L.INGEST_CLASS,
                                                     "CLASS_ALLZERO_IGNORE": L.INGEST_CLASS_ALLZERO_IGNORE,
                                                     "NORMALS": L.INGEST_NORMALS, "DEPTH": L.INGEST_DEPTH}
    assert "#define MTLORA_INGEST_MAX_JOBS 8" in hdr and L.INGEST_MAX_JOBS == 8


def test_device_loader_argument_checks():
    from mtlora_amd import data as D
    ok = dict(batches=[], tasks=["semseg"], device="cuda:0")
    for bad in (dict(flip_p=-0.1), dict(flip_p=1.5), dict(depth=0), dict(depth=1.5), dict(tasks=[]), dict(tasks=["nothing"]),
                dict(tasks=["semseg"] * 8)):
        with pytest.raises(ValueError):
            D.DeviceLoader(**{**ok, **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DeviceLoader(**{**ok, "device": "cpu"})
    dl = D.DeviceLoader([1, 2, 3], ["semseg", "normals"], "cuda:0", flip_p=0.5, seed=3, depth=3)  # (touches no device yet)
    assert (dl.flip_p, dl.seed, dl.depth, len(dl)) == (0.5, 3, 3, 3)
    sig = inspect.signature(D.DeviceLoader.__init__)
    assert list(sig.parameters)[1:7] == ["batches", "tasks", "device", "flip_p", "seed", "depth"]
    assert (sig.parameters["flip_p"].default, sig.parameters["seed"].default, sig.parameters["depth"].default) == (0.0, 0, 2)
    sig = inspect.signature(D.prepare_batch)
    assert list(sig.parameters) == ["batch", "tasks", "flip", "mean", "std"]
    assert sig.parameters["mean"].default == D.IMAGENET_MEAN == (0.485, 0.456, 0.406) and sig.parameters["std"].default == D.IMAGENET_STD


def test_prepare_batch_has_no_cpu_fallback_and_checks_the_wire_format():
    from mtlora_amd import data as D
    from mtlora_amd import functional as Fn
    wire = D.synthetic_wire_batch(2, 8, ALL_TASKS, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.prepare_batch(wire, ALL_TASKS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.ingest_batch([("class", wire["semseg"])])
    for key, bad in (("image", wire["image"].float()), ("image", wire["image"].permute(0, 3, 1, 2)), ("semseg", wire["semseg"].float()),
                     ("sal", wire["sal"][:, :4]), ("normals", wire["normals"].double()), ("normals", wire["normals"][..., :2]),
                     ("depth", wire["depth"].half()), ("flip", torch.zeros(2)), ("flip", torch.zeros(3, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="wire batch"):
            D.prepare_batch_torch({**wire, key: bad}, ALL_TASKS)
    with pytest.raises(ValueError, match="missing"):
        D.prepare_batch_torch({"image": wire["image"]}, ["sal"])
    assert Fn.INGEST_KINDS == {"image": 0, "class": 1, "class_allzero_ignore": 2, "normals": 3, "depth": 4}


def test_synthetic_wire_batch_round_trip():
    """prepare_batch_torch of the synthetic wire batch has the dtypes, shapes and value sets of synthetic_batch"""
    from mtlora_amd import data as D
    from mtlora_amd import mtl_harness as H
    B, S = 3, 32
    wire = D.synthetic_wire_batch(B, S, ALL_TASKS, seed=5)
    assert wire["image"].dtype == torch.uint8 and wire["image"].shape == (B, S, S, 3)
    assert torch.equal(wire["image"], D.synthetic_wire_batch(B, S, ALL_TASKS, seed=5)["image"])  # a seed reproduces it
    assert D.synthetic_wire_batch(B, S, ["normals"], seed=5, normals_dtype=torch.float16)["normals"].dtype == torch.float16
    # numpy arrays are taken as well
    img, tg = D.prepare_batch_torch({k: v.numpy() for k, v in wire.items()}, ALL_TASKS)
    ref_img, ref_tg = H.synthetic_batch(B, S, ALL_TASKS, seed=5)
    assert img.dtype == ref_img.dtype and img.shape == ref_img.shape
    lut = D.image_table()
    assert float(img.min()) >= float(lut.min()) and float(img.max()) <= float(lut.max())
    for t in ALL_TASKS:
        a, r = tg[t], ref_tg[t]
        assert a.dtype == r.dtype == torch.float32 and a.shape == r.shape and a.is_contiguous(), t
        if t in ("semseg", "human_parts", "sal", "edge"):
            assert set(a.unique().tolist()) == set(r.unique().tolist()), t
    for t in ("semseg", "human_parts"):  # 5 % ignored pixels
        assert abs(float((tg[t] == 255).float().mean()) - 0.05) < 0.02
    assert abs(float(tg["sal"].mean()) - 0.3) < 0.05 and abs(float(tg["edge"].mean()) - 0.1) < 0.05
    ign = (tg["normals"] == 255).all(1)
    assert bool(((tg["normals"] == 255).any(1) == ign).all()) and abs(float(ign.float().mean()) - 0.05) < 0.02
    assert bool(((tg["normals"].norm(dim=1) - 1).abs()[~ign] < 1e-5).all())
    assert bool(((ref_tg["normals"] == 255).all(1) == (ref_tg["normals"] == 255).any(1)).all())
    d = tg["depth"]
    assert float(d.min()) >= 0 and bool(((d < 10) | (d == 255)).all()) and float(ref_tg["depth"].max()) < 10
