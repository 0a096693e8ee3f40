"""Checkpoints from the replayed loop on the GPU: mtlora_snapshot_pack / _unpack (csrc/snapshot.hip) against byte views, and
checkpoint.TrainState / save_checkpoint(state=) / load_checkpoint around a GraphedTrainStep with the capturable FusedAdamW, the
in-graph schedule, the fp16 LossScaler and accumulation_steps=2.  Everything here is bit for bit: the kernel copies bytes, and a
resumed run is compared with a run that was stopped and rebuilt the same way through the objects' own state_dict()s.

Model: the smallest the graph tests build (test_gpu_optim_capturable's: 224 px, depths 2-2-2-2, r 16 / 4), with dropout and
drop-path at 0 (RNG state is not checkpointed, as in the reference)."""
import ctypes
import logging
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

LOG = logging.getLogger("test_gpu_snapshot")
POISON, GAP = 0x5A, 0xA5


def dev():
    return torch.device("cuda:0")


def raw(t):
    """the bytes of a tensor, in memory order"""
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_tree(a, b, where=""):
    """equal key for key and type for type; tensors bit for bit (compared on the host)"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b), where
        assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(raw(a).cpu(), raw(b).cpu()), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), (where, list(a.keys())[:8], list(b.keys())[:8])
        for k in a:
            same_tree(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{where}[{i}]")
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
BIG = 12 << 20  # the caching allocator hands a request above 10 MiB to hipMalloc as it is (rounded to 2 MiB): such a tensor's
#                 last byte is the allocation's last byte


def tensor_set(fill):
    """the tensors of the kernel test, in packed order, and the storages some of them are views of.  ``fill(t)`` sets the bytes of
    a freshly allocated tensor.  Built twice (values, then poison): the allocator aligns every allocation to 512 bytes, so the
    two sets agree in every address's alignment."""
    d = dev()
    own = []

    def new(n, dtype=torch.uint8):
        t = torch.empty(n, dtype=dtype, device=d)
        fill(t)
        own.append(t)
        return t

    ts = [new(n) for n in (0, 1, 3, 15, 16, 17, 65537)]  # bytes; 65537 crosses two chunk boundaries and leaves one byte
    ts += [new(30001, torch.float32),  # 120004 bytes: larger than a chunk, a 4-byte tail
           new(777, torch.bfloat16), new(5, torch.int64), new(1, torch.int64).reshape(()), new(0, torch.float32),
           new(4099, torch.float32).reshape(4099, 1)]
    store = new(80000)
    ts += [store[1:1 + 4099], store[40003:40003 + 33001],  # views at odd byte offsets: the byte path, the second across a chunk boundary
           store[4100 + 4:4100 + 4 + 5000]]  # 4-byte aligned, not 16: the dword path
    big_a, big_b = new(BIG), new(BIG)
    ts += [big_a[BIG - 100001:],  # odd start, ends on the allocation's last byte
           big_b[BIG - 8192:]]  # 16-byte aligned, ends on the allocation's last byte: the vector path up to the edge
    return ts, own


def layout(ts):
    off, offs = 0, []
    for t in ts:
        offs.append(off)
        off = -(-(off + t.numel() * t.element_size()) // 16) * 16
    return offs, off


def device_table(L, ts, offs):
    lib = L.lib()
    eb = lib.mtlora_snapshot_entry_bytes()
    host = (ctypes.c_ubyte * (eb * len(ts)))()
    for i, (t, o) in enumerate(zip(ts, offs)):
        nbytes = t.numel() * t.element_size()
        assert t.is_contiguous()
        L.check(lib.mtlora_snapshot_entry(ctypes.byref(host, i * eb), ctypes.c_void_p(t.data_ptr() if nbytes else 0), nbytes, o), "entry")
    n_chunks = lib.mtlora_snapshot_chunks(host, len(ts))
    return torch.frombuffer(host, dtype=torch.uint8).clone().to(dev()), n_chunks


def test_pack_and_unpack_are_byte_exact():
    """pack against torch.cat of byte views (with the 16-byte alignment gaps, which must keep their 0xA5 fill); unpack(pack(x))
    into a poisoned second set restores every tensor and writes nothing around the views"""
    from mtlora_amd import _lib as L
    g = torch.Generator(device="cpu").manual_seed(3)

    def values(t):
        raw(t).copy_(torch.randint(0, 256, (t.numel() * t.element_size(),), dtype=torch.uint8, generator=g))

    ts, own = tensor_set(values)
    offs, extent = layout(ts)
    assert {t.data_ptr() % 16 for t in ts if t.numel()} > {0}  # misaligned sources are really there
    assert any(t.data_ptr() % 4 == 0 and t.data_ptr() % 16 for t in ts) and any(t.data_ptr() % 2 for t in ts)
    table, n_chunks = device_table(L, ts, offs)
    assert n_chunks == -(-extent // L.SNAPSHOT_CHUNK) and n_chunks > 1
    host_table = table.cpu()
    assert L.lib().mtlora_snapshot_check(ctypes.c_void_p(host_table.data_ptr()), len(ts), extent) == 0
    assert L.lib().mtlora_snapshot_check(ctypes.c_void_p(host_table.data_ptr()), len(ts), extent - 1) == -5

    want = torch.full((extent,), GAP, dtype=torch.uint8, device=dev())
    for t, o in zip(ts, offs):
        want[o:o + t.numel() * t.element_size()] = raw(t)
    packed = torch.full((extent + 64,), GAP, dtype=torch.uint8, device=dev())  # 64 guard bytes behind the extent
    L.check(L.lib().mtlora_snapshot_pack(L.ptr(table), len(ts), n_chunks, L.ptr(packed), extent, L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    assert torch.equal(packed[:extent], want)  # every tensor's bytes in place, every gap still 0xA5
    assert bool((packed[extent:] == GAP).all())
    before = [raw(t).clone() for t in ts]

    ts2, own2 = tensor_set(lambda t: raw(t).fill_(POISON))
    assert [t.data_ptr() % 16 for t in ts2] == [t.data_ptr() % 16 for t in ts]
    table2, n_chunks2 = device_table(L, ts2, offs)
    L.check(L.lib().mtlora_snapshot_unpack(L.ptr(table2), len(ts2), n_chunks2, L.ptr(packed), extent, L.stream_ptr()), "unpack")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(ts2, ts)):
        assert a.dtype == b.dtype and torch.equal(raw(a), raw(b)), f"tensor {i} ({b.dtype}, {b.numel()} elements)"
    for t, b in zip(ts, before):
        assert torch.equal(raw(t), b)  # the sources were only read
    assert torch.equal(packed[:extent], want)
    # what lies around the views was not written: everything of the three storages outside them is still poison
    store2, big_a2, big_b2 = own2[-3], own2[-2], own2[-1]
    mask = torch.ones(store2.numel(), dtype=torch.bool, device=dev())
    for lo, n in ((1, 4099), (40003, 33001), (4104, 5000)):
        mask[lo:lo + n] = False
    assert bool((store2[mask] == POISON).all())
    assert bool((big_a2[:BIG - 100001] == POISON).all()) and bool((big_b2[:BIG - 8192] == POISON).all())


# ---- 2. around the replayed train step ---------------------------------------------------------------------------------------------
TASKS = ["semseg", "normals", "sal", "human_parts"]
MODEL_KW = dict(img_size=224, tasks=TASKS, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, dropout=0.0, seed=4)
K = 2  # accumulation steps


@pytest.fixture(scope="module")
def batches():
    from mtlora_amd import mtl_harness as H
    return [H.synthetic_batch(2, 224, TASKS, seed=100 + i, device=dev()) for i in range(8)]  # batch i feeds replay i of a run


class Run:
    """fresh model, capturable FusedAdamW, linear schedule (exact on the device), fp16 LossScaler -- from fixed seeds"""

    def __init__(self, batches):
        from mtlora_amd import functional as Fn
        from mtlora_amd import lr_scheduler as S
        from mtlora_amd import mtl_harness as H
        from mtlora_amd.optim import LossScaler
        torch.manual_seed(9)
        Fn._seed_counter = 0
        self.batches = batches
        self.model = H.build_model(**MODEL_KW).to(dev()).train()
        self.crit = H.MultiTaskLoss(TASKS)
        self.opt = H.build_optimizer(self.model, lr=1e-3, impl="hip", capturable=True)
        self.sched = S.LinearLRScheduler(self.opt, t_initial=40, lr_min_rate=0.01, warmup_t=3, warmup_lr_init=1e-7, t_in_epochs=False)
        self.scaler = LossScaler(init_scale=2.0 ** 10)
        self.img = batches[0][0].clone()
        self.tg = {t: v.clone() for t, v in batches[0][1].items()}
        self.gs = None

    def capture(self):
        from mtlora_amd import mtl_harness as H
        self.gs = H.GraphedTrainStep(self.model, self.crit, self.opt, self.img, self.tg, clip_grad=5.0, warmup=2, amp_dtype=torch.float16,
                                     loss_scaler=self.scaler, accumulation_steps=K, lr_scheduler=self.sched)
        assert self.gs.graphed is True and self.gs.why == "", self.gs.why
        return self

    def replay(self, indices):
        for i in indices:
            self.img.copy_(self.batches[i][0])
            for t in self.tg:
                self.tg[t].copy_(self.batches[i][1][t])
            self.gs()

    def state(self):
        """the reference: the objects' own state_dict()s (they synchronise), as host copies, plus the raw counters"""
        def host(x):
            if torch.is_tensor(x):
                return x.detach().cpu().clone()
            if isinstance(x, dict):
                return type(x)((k, host(v)) for k, v in x.items())
            if isinstance(x, (list, tuple)):
                return type(x)(host(v) for v in x)
            return x
        torch.cuda.synchronize()
        return {"model": host(dict(self.model.state_dict())), "optimizer": host(self.opt.state_dict()),
                "scaler": self.scaler.state_dict(), "lr_scheduler": host(dict(self.sched.state_dict())),
                "step": self.opt._ctrl[4].item(), "updates": self.opt.num_updates().item(),
                "words": (self.scaler._scale.item(), self.scaler._growth_tracker.item())}


def cfg(out, resume=""):
    ns = types.SimpleNamespace
    return ns(OUTPUT=str(out), EVAL_MODE=False, MODEL=ns(RESUME=str(resume), RESUME_BACKBONE="", MTLORA=ns(ENABLED=False),
                                                        UPDATE_RELATIVE_POSITION=False),
              TRAIN=ns(SKIP_DECODER_CKPT=False, START_EPOCH=0))


_stopped = {}


def stopped(batches, s, out):
    """a run stopped after s replays: its checkpoint, written from a TrainState snapshot by the background thread, and the
    reference state_dict()s taken at the same point (cached: the consistency test and the resume test share the s = 3 run)"""
    from mtlora_amd import checkpoint as C
    from mtlora_amd import functional as Fn
    if s not in _stopped:
        try:
            run = Run(batches).capture()
            ts = C.TrainState(run.model, run.opt, run.sched, run.scaler)
            run.replay(range(s))
            path = C.save_checkpoint(cfg(out), s, run.model, 12.5, run.opt, run.sched, run.scaler, LOG, state=ts, blocking=False)
            C.wait_for_saves()
            _stopped[s] = (path, run.state())
        finally:
            Fn.set_seed_offset(None)
    return _stopped[s]


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    yield tmp_path_factory.mktemp("ckpt")
    _stopped.clear()


def test_snapshot_is_consistent_under_replay(batches, out_dir):
    """3 replays, snapshot(), 3 more replays WITHOUT waiting, then wait(): handle.state() is, bit for bit and key for key, what the
    state_dict()s of a twin run stopped after 3 replays return -- the later replays did not tear it.  The frozen tensors are
    copied once and shared by the next handle; a third snapshot supersedes the first."""
    from mtlora_amd import checkpoint as C
    from mtlora_amd import functional as Fn
    _, twin = stopped(batches, 3, out_dir)
    try:
        run = Run(batches).capture()
        ts = C.TrainState(run.model, run.opt, run.sched, run.scaler)
        run.replay(range(3))
        handle = ts.snapshot()
        run.replay(range(3, 6))
        handle.wait()
        assert handle.ready()
        got, keep = handle.state(), handle.state(copy=True)  # views of the pinned buffer; copies that outlive the handle
        assert list(got.keys()) == ["model", "optimizer", "scaler", "lr_scheduler"]
        assert all(not v.is_cuda for v in got["model"].values())
        same_tree(dict(got["model"]), twin["model"], "model")
        same_tree(got["optimizer"], twin["optimizer"], "optimizer")
        same_tree(got["scaler"], twin["scaler"], "scaler")
        same_tree(dict(got["lr_scheduler"]), twin["lr_scheduler"], "lr_scheduler")
        assert type(got["optimizer"]["lr_schedule_updates"]) is int and got["optimizer"]["lr_schedule_updates"] == twin["updates"] == 3
        assert type(got["scaler"]["scale"]) is float and type(got["scaler"]["_growth_tracker"]) is int
        assert got["optimizer"]["state"][0]["step"].item() == twin["step"] == 3.0  # 2 warm-up steps + the update of replay 2
        assert run.opt._ctrl[4].item() == 5.0  # while the live run went on (updates at replays 2, 4 and 6)

        frozen = [k for k, v in run.model.state_dict(keep_vars=True).items() if isinstance(v, torch.nn.Parameter) and not v.requires_grad]
        assert frozen
        second = ts.snapshot()
        st2 = second.state()
        assert all(st2["model"][k] is got["model"][k] for k in frozen)  # copied to the host once
        same_tree(dict(handle.state()["model"]), twin["model"], "the first handle after a second snapshot")
        ts.snapshot().wait()
        with pytest.raises(RuntimeError, match="superseded"):
            handle.state()

        # a changed trainable set is an error, not a silently stale table
        p = next(p for p in run.model.parameters() if not p.requires_grad)
        p.requires_grad_(True)
        with pytest.raises(RuntimeError, match="trainable parameters changed"):
            ts.snapshot()
        p.requires_grad_(False)

        # restore(): back to the state of replay 3 through the objects' load_state_dict; the accumulation cycle starts over
        ts.restore(keep)
        after = run.state()
        same_tree(after["model"], twin["model"], "restored model")
        same_tree(after["optimizer"], twin["optimizer"], "restored optimizer")
        same_tree(after["scaler"], twin["scaler"], "restored scaler")
        assert run.opt._ctrl[5].item() == 0.0
    finally:
        Fn.set_seed_offset(None)


@pytest.mark.parametrize("s", [3, 4], ids=["mid_cycle", "on_boundary"])
def test_resume_continues_bit_for_bit(batches, out_dir, s):
    """A run is stopped after s replays (s = 3: in the middle of an accumulation cycle of 2; s = 4: on its boundary), saved with
    save_checkpoint(state=TrainState, blocking=False) + wait_for_saves(), and resumed: fresh model, optimizer, scheduler and
    scaler, load_checkpoint, a new GraphedTrainStep, 3 more replays.  Every parameter and buffer, both moments, the step and
    schedule counts and the scaler's words are bit-equal to run A.

    Run A is NOT 6 uninterrupted replays: a GraphedTrainStep's construction makes two eager warm-up steps, which are update calls
    (they move the parameters, the step count and the schedule count), and loading starts a new accumulation cycle (the half-made
    cycle of s = 3 is dropped, as FusedAdamW.load_state_dict documents).  So A is stopped at the same replay, rebuilt the same way
    -- fresh objects, a new GraphedTrainStep with its warm-up -- and continued, but through the objects' own state_dict() /
    load_state_dict() in memory: no TrainState, no snapshot kernel, no file.  The comparison is exact, not a tolerance."""
    from mtlora_amd import checkpoint as C
    from mtlora_amd import functional as Fn
    path, ref = stopped(batches, s, out_dir)
    assert os.path.basename(path) == f"ckpt_epoch_{s}.pth" and C.auto_resume_helper(str(out_dir)) is not None

    file = torch.load(path, map_location="cpu", weights_only=False)  # the file is the reference state, key for key
    assert list(file.keys()) == ["model", "optimizer", "lr_scheduler", "max_accuracy", "scaler", "epoch", "config"]
    same_tree(dict(file["model"]), ref["model"], "file/model")
    same_tree(file["optimizer"], ref["optimizer"], "file/optimizer")
    same_tree(file["scaler"], ref["scaler"], "file/scaler")
    same_tree(dict(file["lr_scheduler"]), ref["lr_scheduler"], "file/lr_scheduler")
    assert ref["updates"] == 2 + s // K and ref["step"] == 2.0 + s // K

    def load_in_memory(run):
        run.model.load_state_dict(ref["model"])
        run.opt.load_state_dict(ref["optimizer"])
        run.sched.load_state_dict(ref["lr_scheduler"])
        run.scaler.load_state_dict(ref["scaler"])

    def load_file(run):
        c = cfg(out_dir, resume=path)
        assert C.load_checkpoint(c, run.model, run.opt, run.sched, run.scaler, LOG) == 12.5
        assert c.TRAIN.START_EPOCH == s + 1

    ends = {}
    for name, load in (("A", load_in_memory), ("B", load_file)):
        try:
            run = Run(batches)
            load(run)
            run.capture()
            assert run.opt.num_updates().item() == ref["updates"] + 2  # the warm-up's two update calls, on top of the loaded count
            run.replay(range(s, s + 3))
            ends[name] = run.state()
        finally:
            Fn.set_seed_offset(None)
    a, b = ends["A"], ends["B"]
    assert a["updates"] == ref["updates"] + 2 + 1 and a["step"] == ref["step"] + 2 + 1  # 3 replays from c = 0: one update
    for key in ("model", "optimizer", "scaler", "lr_scheduler"):
        same_tree(b[key], a[key], key)
    assert b["step"] == a["step"] and b["updates"] == a["updates"] and b["words"] == a["words"]
    moved = [k for k in a["model"] if a["model"][k].is_floating_point() and not torch.equal(a["model"][k], ref["model"][k])]
    assert moved  # the continuation trained


def test_adapter_only_snapshot_file(batches, out_dir):
    """save_checkpoint(state=, trainable_only=True): the file holds the trainable parameters and the buffers only, bit-equal to
    the model's"""
    from mtlora_amd import checkpoint as C
    full_path, ref = stopped(batches, 3, out_dir)
    model = Run(batches).model
    model.load_state_dict(ref["model"])
    ts = C.TrainState(model)
    sub = out_dir / "adapter"
    sub.mkdir()
    path = C.save_checkpoint(cfg(sub), 0, model, 0.0, None, None, None, LOG, state=ts, trainable_only=True)
    file = torch.load(path, map_location="cpu", weights_only=False)
    assert file["trainable_only"] is True and file["optimizer"] is None
    want = C.lora_state_dict(model)
    assert list(file["model"].keys()) == list(want.keys())
    same_tree(dict(file["model"]), {k: v for k, v in want.items()}, "adapter-only model")
    n_frozen = sum(1 for p in model.parameters() if not p.requires_grad)
    assert n_frozen and len(file["model"]) == len(model.state_dict()) - n_frozen
    assert os.path.getsize(path) < os.path.getsize(full_path)


def test_torch_optimizer_and_meters_are_part_of_the_snapshot():
    """a torch AdamW (state enumerated lazily, at the first snapshot after a step) and a meter bank: handle.state() equals the
    objects' own state after one step and, through a rebuilt table, after the optimizer's state came into being"""
    from mtlora_amd import checkpoint as C
    from mtlora_amd.meters import TrainMeters
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.BatchNorm1d(17), torch.nn.Linear(17, 5)).to(dev()).train()
    model[0].weight.requires_grad_(False)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-2, fused=True)
    value = torch.zeros((), dtype=torch.float32, device=dev())
    meters = TrainMeters(dev()).add("value", value).seal()
    ts = C.TrainState(model, opt, None, None, meters)

    def check(handle):
        got = handle.state()
        torch.cuda.synchronize()
        same_tree(dict(got["model"]), dict(model.state_dict()), "model")
        same_tree(got["optimizer"], opt.state_dict(), "optimizer")
        assert got["scaler"] is None and "lr_scheduler" not in got
        assert torch.equal(got["meters"]["bank"], meters.bank.cpu()) and got["meters"]["counter"] == meters.counter.item()

    check(ts.snapshot())  # before the first step: the optimizer has no state yet
    for i in range(2):
        model(torch.randn(8, 33, device=dev())).square().mean().backward()
        opt.step()
        opt.zero_grad()
        value.fill_(1.5 + i)
        meters.update()
        h = ts.snapshot()
        assert len(h.state()["optimizer"]["state"]) == 5
        check(h)
    assert ts.snapshot().state()["meters"]["counter"] == 2
    model[2].weight.data = model[2].weight.data.clone()  # a re-allocated parameter: the table's address is stale
    with pytest.raises(RuntimeError, match="re-allocated"):
        ts.snapshot()
