"""Saving checkpoints (mtlora_amd/checkpoint.py: save_checkpoint, auto_resume_helper, lora_state_dict / trainable_only, after
reference utils.py:280-321) and what the snapshot entry points (csrc/snapshot.hip) decide BEFORE any launch -- no GPU needed."""
import ctypes
import logging
import os
import re
import types

import pytest
import torch
import torch.nn as nn

OK, SHAPE, ALIGN, NULL, WORKSPACE = 0, -2, -3, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = logging.getLogger("test_cpu_checkpoint_save")


@pytest.fixture(scope="module")
def L():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    _lib.lib()
    return _lib


# ---- 1. the C ABI: validation with null device pointers -------------------------------------------------------------------------
FAKE = 0x7F0000001000  # an address that is never dereferenced: every call below returns before a launch, or only writes the host table


def table(L, rows):
    """a host table of (address, bytes, packed offset) rows; returns the buffer and the statuses mtlora_snapshot_entry gave"""
    eb = L.lib().mtlora_snapshot_entry_bytes()
    host = (ctypes.c_ubyte * (eb * max(len(rows), 1)))()
    st = [L.lib().mtlora_snapshot_entry(ctypes.byref(host, i * eb), ctypes.c_void_p(p), b, o) for i, (p, b, o) in enumerate(rows)]
    return host, st


def test_entry_size_and_entry_validation(L):
    assert L.lib().mtlora_snapshot_entry_bytes() == 32
    _, st = table(L, [(FAKE, 5, 0), (FAKE, -1, 16), (FAKE, 4, 8), (0, 4, 16), (0, 0, 16), (FAKE, 4, -16)])
    assert st == [OK, SHAPE, ALIGN, NULL, OK, SHAPE]  # negative size; offset off 16; null address with bytes; a null empty tensor is legal
    assert L.lib().mtlora_snapshot_entry(None, ctypes.c_void_p(FAKE), 4, 0) == NULL


def test_chunks_counts_the_packed_extent_and_accepts_a_zero_byte_entry(L):
    C = L.SNAPSHOT_CHUNK
    lib = L.lib()
    assert lib.mtlora_snapshot_chunks(None, 0) == 0
    host, st = table(L, [(FAKE, 3, 0), (0, 0, 16), (FAKE, 17, 16), (FAKE, C, 48)])
    assert st == [OK] * 4
    assert lib.mtlora_snapshot_chunks(host, 4) == 2  # the extent is 48 + C: one whole chunk and 48 bytes of the next
    assert lib.mtlora_snapshot_chunks(host, 3) == 1
    assert lib.mtlora_snapshot_chunks(host, 2) == 1
    host, _ = table(L, [(0, 0, 0)])
    assert lib.mtlora_snapshot_chunks(host, 1) == 0  # nothing but an empty tensor: nothing to launch
    host, _ = table(L, [(FAKE, C, 0), (FAKE, 1, C)])
    assert lib.mtlora_snapshot_chunks(host, 2) == 2 and lib.mtlora_snapshot_chunks(host, 1) == 1


def test_table_validation(L):
    lib = L.lib()
    assert lib.mtlora_snapshot_chunks(None, 3) == NULL  # null table with n > 0
    assert lib.mtlora_snapshot_chunks(None, -1) == SHAPE
    host, st = table(L, [(FAKE, 20, 0), (FAKE, 4, 16)])  # the second entry begins inside the first
    assert st == [OK, OK]
    assert lib.mtlora_snapshot_chunks(host, 2) == SHAPE and lib.mtlora_snapshot_check(host, 2, 1 << 20) == SHAPE
    host, _ = table(L, [(FAKE, 4, 32), (FAKE, 4, 0)])  # not in packed order
    assert lib.mtlora_snapshot_chunks(host, 2) == SHAPE
    host, _ = table(L, [(FAKE, 20, 0), (FAKE, 4, 32)])
    assert lib.mtlora_snapshot_chunks(host, 2) == 1
    assert lib.mtlora_snapshot_check(host, 2, 36) == OK
    assert lib.mtlora_snapshot_check(host, 2, 35) == WORKSPACE  # packed_bytes smaller than the table's extent
    assert lib.mtlora_snapshot_check(host, 2, -1) == SHAPE
    assert lib.mtlora_snapshot_check(None, 2, 64) == NULL
    # an entry written by hand with an offset off 16 (mtlora_snapshot_entry refuses to write one)
    raw = (ctypes.c_int64 * 4)(FAKE, 4, 8, 0)
    assert lib.mtlora_snapshot_chunks(raw, 1) == ALIGN and lib.mtlora_snapshot_check(raw, 1, 64) == ALIGN
    raw = (ctypes.c_int64 * 4)(FAKE, -4, 0, 0)
    assert lib.mtlora_snapshot_chunks(raw, 1) == SHAPE


@pytest.mark.parametrize("fn", ["mtlora_snapshot_pack", "mtlora_snapshot_unpack"])
def test_launch_validation_comes_before_any_launch(L, fn):
    """every rejection below returns before a launch: the table and packed addresses are never dereferenced (there is no GPU)"""
    C = L.SNAPSHOT_CHUNK
    f = getattr(L.lib(), fn)
    T, P = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE + 0x100000)
    assert f(None, 2, 1, P, C, None) == NULL  # null table with n > 0
    assert f(T, 2, 1, None, C, None) == NULL  # null packed with chunks to copy
    assert f(T, -1, 1, P, C, None) == SHAPE
    assert f(T, 2, -1, P, C, None) == SHAPE
    assert f(T, 2, 1, P, -1, None) == SHAPE
    assert f(T, 2, 3, P, 2 * C, None) == WORKSPACE  # three chunks cover more than two whole ones
    assert f(T, 2, 1, P, 0, None) == WORKSPACE
    assert f(ctypes.c_void_p(FAKE + 4), 2, 1, P, C, None) == ALIGN
    assert f(T, 2, 1, ctypes.c_void_p(FAKE + 8), C, None) == ALIGN
    assert f(None, 0, 0, None, 0, None) == OK  # an empty table: nothing to do, nothing launched
    assert f(T, 2, 0, None, 0, None) == OK  # only empty tensors


def test_new_prototypes_match_the_ctypes_signatures(L):
    """the six snapshot prototypes of the header, parameter for parameter, against _lib._SIGS"""
    hdr = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {n: (r, a) for r, n, a in re.findall(r"\b(int64_t|int)\s+(mtlora_snapshot_[a-z_]+)\s*\(([^;{}]*?)\)\s*;", hdr)}
    names = {"mtlora_snapshot_entry_bytes", "mtlora_snapshot_entry", "mtlora_snapshot_chunks", "mtlora_snapshot_check",
             "mtlora_snapshot_pack", "mtlora_snapshot_unpack"}
    assert set(protos) == names and names <= set(L.EXPORTS)
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}
    for name in names:
        res, args = L._SIGS[name]
        ret, params = protos[name]
        assert ctype[ret] is res, name
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        want = [ctypes.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
        assert want == list(args), (name, params)
    assert int(re.search(r"#define MTLORA_SNAPSHOT_CHUNK (\d+)", hdr).group(1)) == L.SNAPSHOT_CHUNK
    assert "snapshot.hip" in __import__("mtlora_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


# ---- 2. save_checkpoint / load_checkpoint / auto_resume_helper on the host --------------------------------------------------------
class Tiny(nn.Module):
    """a frozen linear with a trainable adapter and a BatchNorm: frozen parameters, trainable ones and buffers"""

    def __init__(self):
        super().__init__()
        self.base = nn.Linear(6, 5)
        self.lora_A = nn.Parameter(torch.randn(2, 6))
        self.lora_B = nn.Parameter(torch.randn(5, 2))
        self.bn = nn.BatchNorm1d(5)
        for p in self.base.parameters():
            p.requires_grad_(False)

    def forward(self, x):
        return self.bn(self.base(x) + x @ self.lora_A.t() @ self.lora_B.t())


def cfg(out, resume=""):
    ns = types.SimpleNamespace
    return ns(OUTPUT=str(out), EVAL_MODE=False, MODEL=ns(RESUME=str(resume), RESUME_BACKBONE="", MTLORA=ns(ENABLED=False),
                                                        UPDATE_RELATIVE_POSITION=False),
              TRAIN=ns(SKIP_DECODER_CKPT=False, START_EPOCH=0))


def trained(seed, steps=3):
    torch.manual_seed(seed)
    model = Tiny()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    scaler = torch.amp.GradScaler("cpu", enabled=True, init_scale=128.0)
    for _ in range(steps):
        model(torch.randn(8, 6)).square().mean().backward()
        opt.step()
        opt.zero_grad()
        sched.step()
    return model, opt, sched, scaler


def same_tree(a, b, where=""):
    """equal key for key; tensors bit for bit"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b), where
        assert a.dtype == b.dtype and a.shape == b.shape, where
        assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)) if a.numel() else True, where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), (where, list(a.keys()), list(b.keys()))
        for k in a:
            same_tree(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{where}[{i}]")
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def test_save_and_load_round_trip(tmp_path):
    from mtlora_amd import checkpoint as C
    model, opt, sched, scaler = trained(0)
    path = C.save_checkpoint(cfg(tmp_path), 7, model, 61.5, opt, sched, scaler, LOG)
    assert path == os.path.join(str(tmp_path), "ckpt_epoch_7.pth") and os.path.isfile(path)
    assert sorted(os.listdir(tmp_path)) == ["ckpt_epoch_7.pth"]  # no temporary file is left
    raw = torch.load(path, map_location="cpu", weights_only=False)  # plain torch.load
    assert list(raw.keys()) == ["model", "optimizer", "lr_scheduler", "max_accuracy", "scaler", "epoch", "config"]
    assert raw["epoch"] == 7 and raw["max_accuracy"] == 61.5 and raw["config"].OUTPUT == str(tmp_path)
    same_tree(dict(raw["model"]), dict(model.state_dict()), "model")
    same_tree(raw["optimizer"], opt.state_dict(), "optimizer")
    same_tree(raw["lr_scheduler"], sched.state_dict(), "lr_scheduler")
    same_tree(raw["scaler"], scaler.state_dict(), "scaler")

    model2, opt2, sched2, scaler2 = trained(1, steps=1)  # other values, and one step so that the optimizer has state to replace
    c2 = cfg(tmp_path, resume=path)
    assert C.load_checkpoint(c2, model2, opt2, sched2, scaler2, LOG) == 61.5
    assert c2.TRAIN.START_EPOCH == 8
    same_tree(dict(model2.state_dict()), dict(model.state_dict()), "model")
    same_tree(opt2.state_dict(), opt.state_dict(), "optimizer")
    same_tree(sched2.state_dict(), sched.state_dict(), "lr_scheduler")
    same_tree(scaler2.state_dict(), scaler.state_dict(), "scaler")


def test_auto_resume_helper(tmp_path):
    from mtlora_amd import checkpoint as C
    assert C.auto_resume_helper(str(tmp_path)) is None
    (tmp_path / "notes.txt").write_text("not a checkpoint")
    (tmp_path / "ckpt_epoch_9.pth.tmp").write_text("a write in progress")
    assert C.auto_resume_helper(str(tmp_path)) is None
    for name, mtime in (("ckpt_epoch_2.pth", 3000), ("ckpt_epoch_10.pth", 2000), ("ckpt_epoch_1.pth", 1000)):
        (tmp_path / name).write_bytes(b"x")
        os.utime(tmp_path / name, (mtime, mtime))
    assert C.auto_resume_helper(str(tmp_path)) == os.path.join(str(tmp_path), "ckpt_epoch_2.pth")  # by mtime, not by name
    os.utime(tmp_path / "ckpt_epoch_1.pth", (4000, 4000))
    assert C.auto_resume_helper(str(tmp_path)) == os.path.join(str(tmp_path), "ckpt_epoch_1.pth")


def test_adapter_only_file(tmp_path):
    from mtlora_amd import checkpoint as C
    model, opt, sched, scaler = trained(0)
    want = ["lora_A", "lora_B", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    names = [n for n, p in model.named_parameters() if p.requires_grad] + [n for n, _ in model.named_buffers()]
    assert sorted(names) == sorted(want)
    lsd = C.lora_state_dict(model)
    assert sorted(lsd.keys()) == sorted(want) and all(not v.requires_grad for v in lsd.values())
    same_tree({k: lsd[k] for k in lsd}, {k: v for k, v in model.state_dict().items() if k in lsd}, "lora_state_dict")

    path = C.save_checkpoint(cfg(tmp_path), 0, model, 1.0, opt, sched, scaler, LOG, trainable_only=True)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert list(raw.keys()) == ["model", "optimizer", "lr_scheduler", "max_accuracy", "scaler", "epoch", "config", "trainable_only"]
    assert raw["trainable_only"] is True and sorted(raw["model"].keys()) == sorted(want)

    torch.manual_seed(5)
    fresh, opt2, sched2, scaler2 = trained(5, steps=1)
    base_before = {k: v.clone() for k, v in fresh.base.state_dict().items()}
    seen = []
    log = types.SimpleNamespace(info=lambda m: seen.append(("info", m)), warning=lambda m: seen.append(("warning", m)))
    C.load_checkpoint(cfg(tmp_path, resume=path), fresh, opt2, sched2, scaler2, log)
    for k in want:
        same_tree(fresh.state_dict()[k], model.state_dict()[k], k)
    same_tree(dict(fresh.base.state_dict()), base_before, "frozen tensors keep their values")
    assert any(kind == "info" and "2 frozen tensors" in m and "expected" in m for kind, m in seen), seen
    assert not any(kind == "warning" for kind, m in seen), seen  # the missing frozen keys are not reported as a problem
    same_tree(opt2.state_dict(), opt.state_dict(), "optimizer")

    raw["model"]["lora_C"] = torch.zeros(1)  # an unexpected key is still an error
    bad = os.path.join(str(tmp_path), "bad.pth")
    torch.save(raw, bad)
    with pytest.raises(RuntimeError, match="lora_C"):
        C.load_checkpoint(cfg(tmp_path, resume=bad), fresh, opt2, sched2, scaler2, log)


def test_failed_background_write_is_raised(tmp_path):
    """the writer's failure surfaces at wait_for_saves() (and is cleared by it); exercised through the module's own queue"""
    from mtlora_amd import checkpoint as C
    import concurrent.futures
    C.wait_for_saves()  # nothing pending: returns
    ex = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    with C._pending_lock:
        C._pending.append(ex.submit(C._write, {"x": 1}, os.path.join(str(tmp_path), "no_such_dir", "ckpt_epoch_0.pth"), LOG))
    with pytest.raises(RuntimeError, match="background checkpoint write failed"):
        C.wait_for_saves()
    C.wait_for_saves()
    ex.shutdown()


def test_train_state_needs_a_gpu():
    from mtlora_amd import checkpoint as C
    with pytest.raises(RuntimeError, match="GPU"):
        C.TrainState(Tiny())
