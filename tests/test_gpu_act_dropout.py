"""Activation dropout (MODEL.DROP_RATE) on the HIP path: the two kernel families through the C ABI against their fp64 restatement with
the oracle's generator, the block against its nn.Dropout path with the same masks, the ATen ops that must be gone, and graph replay.
Tolerances: those of tests/test_gpu_kernels.py (relative to max |ref|), at 1x."""
import ctypes
import math

import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2, torch.float16: 2e-3}  # tests/test_gpu_kernels.py
HIDDEN, PROJ, MLP_OUT, POS, STRIDE = 0x42, 0x43, 0x44, 0x45, 0x100
SEED = 0x5EED_0000_FFFF_FFFF  # (seed + 1 carries into the high word)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def check(a, ref, dtype, what):
    e = rel_err(a, ref)
    print(f"{what}: rel err {e:.3e} (tol {TOL[dtype]:.0e})")
    assert e <= TOL[dtype], f"{what}: rel err {e:.3e} > {TOL[dtype]:.1e}"


def _drop(p, seed=SEED, off=None):
    from mtlora_amd import _lib as L
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = p, seed, (None if off is None else off.data_ptr())
    return dr


def _keep(site, k, M, C, p, seed=SEED):
    return O.dropout_keep_mask_t(seed, site + STRIDE * k, M, C, p, device=dev())


def _gelu64(h):
    return 0.5 * h * (1 + torch.erf(h / math.sqrt(2.0)))


def _gelu_grad64(h):
    return 0.5 * (1 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def _act_abi(hs, gs, p, site, act, dr=None):
    """(a list, dh list) of mtlora_act_dropout_fwd / _bwd; outputs start as NaN so that an unwritten element shows"""
    from mtlora_amd import _lib as L
    n, (M, C), dt = len(hs), hs[0].shape, hs[0].dtype
    dr = dr or _drop(p)
    a = [torch.full_like(h, float("nan")) for h in hs]
    dh = [torch.full_like(h, float("nan")) for h in hs]
    lib, P9 = L.lib(), L.ptr_array9
    L.check(lib.mtlora_act_dropout_fwd(n, P9(hs), P9(a), ctypes.byref(dr), site, act, M, C, L.dtype_code(hs[0]), L.stream_ptr()), "fwd")
    L.check(lib.mtlora_act_dropout_bwd(n, P9(gs), P9(hs) if act else None, P9(dh), ctypes.byref(dr), site, act, M, C, L._DT[dt],
                                       L.stream_ptr()), "bwd")
    return a, dh


# ---- 1. drop(act(h)) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", [96, 384])
def test_act_dropout_against_fp64(C, act, dtype):
    M = 2 * 49 + 3  # no multiple of any rows-per-workgroup: the tail of the last workgroup is partial
    torch.manual_seed(C + act)
    for n in (1, 5, 9):
        hs = [torch.randn(M, C, device=dev()).mul_(1.5).to(dtype) for _ in range(n)]
        gs = [torch.randn(M, C, device=dev()).to(dtype) for _ in range(n)]
        for p in (0.1, 0.5):
            site = HIDDEN if act else POS
            a, dh = _act_abi(hs, gs, p, site, act)
            for k in range(n):
                keep = _keep(site, k, M, C, p)
                assert 0.6 * (1 - p) < keep.float().mean().item() < min(1.0, 1.4 * (1 - p))
                h64, g64 = hs[k].double(), gs[k].double()
                ref = torch.where(keep, (_gelu64(h64) if act else h64) / (1 - p), 0.0)
                dref = torch.where(keep, g64 * (_gelu_grad64(h64) if act else 1.0) / (1 - p), 0.0)
                assert bool((a[k][~keep] == 0).all()) and bool((dh[k][~keep] == 0).all()), (n, p, k)
                assert bool(torch.isfinite(a[k].float()).all()) and bool(torch.isfinite(dh[k].float()).all())
                check(a[k], ref, dtype, f"a n={n} p={p} k={k}")
                check(dh[k], dref, dtype, f"dh n={n} p={p} k={k}")
            if n > 1:  # every tensor of a call has its own mask
                assert not torch.equal(_keep(site, 0, M, C, p), _keep(site, 1, M, C, p))


def test_act_dropout_p_zero_seed_and_offset():
    """p == 0: act(h) alone (for the identity: a bit-exact copy); the same seed twice: the same bits; seed_offset = 1: seed + 1"""
    M, C, n = 101, 96, 3
    torch.manual_seed(3)
    for dtype in (torch.float32, torch.bfloat16):
        hs = [torch.randn(M, C, device=dev()).to(dtype) for _ in range(n)]
        gs = [torch.randn(M, C, device=dev()).to(dtype) for _ in range(n)]
        a, dh = _act_abi(hs, gs, 0.0, POS, 0)
        assert all(torch.equal(x, h) for x, h in zip(a, hs)) and all(torch.equal(x, g) for x, g in zip(dh, gs))
        a, _ = _act_abi(hs, gs, 0.0, HIDDEN, 1)
        check(a[0], _gelu64(hs[0].double()), dtype, "gelu at p = 0")
        r1, r2 = _act_abi(hs, gs, 0.3, HIDDEN, 1), _act_abi(hs, gs, 0.3, HIDDEN, 1)
        assert all(torch.equal(x, y) for x, y in zip(r1[0] + r1[1], r2[0] + r2[1]))
        off = torch.ones(1, dtype=torch.int64, device=dev())
        r3 = _act_abi(hs, gs, 0.3, HIDDEN, 1, _drop(0.3, SEED, off))
        r4 = _act_abi(hs, gs, 0.3, HIDDEN, 1, _drop(0.3, SEED + 1))
        assert all(torch.equal(x, y) for x, y in zip(r3[0] + r3[1], r4[0] + r4[1]))
        assert not torch.equal(r1[0][0], r3[0][0])


# ---- 2. residual + DropPath + dropout -------------------------------------------------------------------------------------------------
def _res_abi(res, ys, gs, scale, B, dr, shared, plain=False):
    from mtlora_amd import _lib as L
    n, (M, C) = len(ys), ys[0].shape
    rlist = [res[0]] * n if shared else res
    outs = [torch.full_like(rlist[0], float("nan")) for _ in range(n)]
    dys = [torch.full_like(y, float("nan")) for y in ys]
    dres = torch.full_like(rlist[0], float("nan")) if shared else None
    lib, P9 = L.lib(), L.ptr_array9
    rc, yc, s = L.dtype_code(rlist[0]), L.dtype_code(ys[0]), L.stream_ptr()
    if plain:
        L.check(lib.mtlora_residual_droppath_fwd(n, P9(rlist), P9(ys), P9(outs), L.ptr(scale), M, C, B, rc, yc, s), "fwd")
        L.check(lib.mtlora_residual_droppath_bwd(n, P9(gs), P9(dys), L.ptr(dres), L.ptr(scale), M, C, B, rc, yc, s), "bwd")
    else:
        L.check(lib.mtlora_residual_droppath_drop_fwd(n, P9(rlist), P9(ys), P9(outs), L.ptr(scale), ctypes.byref(dr), PROJ, M, C, B, rc, yc,
                                                      s), "drop fwd")
        L.check(lib.mtlora_residual_droppath_drop_bwd(n, P9(gs), P9(dys), L.ptr(dres), L.ptr(scale), ctypes.byref(dr), PROJ, M, C, B, rc, yc,
                                                      s), "drop bwd")
    return outs, dys, dres


@pytest.mark.parametrize("rdt,ydt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                                     (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("M,B", [(2 * 49 + 3, 1), (2 * 3136, 2)])
def test_residual_droppath_drop_against_fp64(M, B, rdt, ydt):
    torch.manual_seed(M)
    for C, n, p, shared, scaled in ((96, 1, 0.1, False, False), (96, 5, 0.5, True, True), (384, 9, 0.1, False, True),
                                    (384, 5, 0.5, True, False), (96, 9, 0.1, True, True), (384, 1, 0.5, False, True)):
        res = [torch.randn(M, C, device=dev()).to(rdt) for _ in range(1 if shared else n)]
        ys = [torch.randn(M, C, device=dev()).to(ydt) for _ in range(n)]
        gs = [torch.randn(M, C, device=dev()).to(rdt) for _ in range(n)]
        scale = None
        if scaled:
            scale = ((torch.rand(n, B, device=dev()) < 0.7).float() / 0.7).contiguous()
            scale[0, 0] = 1.0 / 0.7
        outs, dys, dres = _res_abi(res, ys, gs, scale, B, _drop(p), shared)
        for k in range(n):
            keep = _keep(PROJ, k, M, C, p)
            s64 = 1.0 if scale is None else scale[k].double().repeat_interleave(M // B).unsqueeze(-1)
            r = res[0] if shared else res[k]
            ref = r.double() + s64 * torch.where(keep, ys[k].double() / (1 - p), 0.0)
            dref = s64 * torch.where(keep, gs[k].double() / (1 - p), 0.0)
            assert torch.equal(outs[k][~keep], r[~keep]), (C, n, p, k)  # dropped: the residual, bit for bit
            assert bool((dys[k][~keep] == 0).all()), (C, n, p, k)
            check(outs[k], ref, rdt, f"out C={C} n={n} p={p} k={k}")
            check(dys[k], dref, ydt, f"dy C={C} n={n} p={p} k={k}")
        if shared:
            check(dres, sum(g.double() for g in gs), rdt, f"dres C={C} n={n}")


def test_residual_droppath_drop_p_zero_seed_and_offset():
    M, C, n, B = 2 * 49 + 3, 96, 3, 1
    torch.manual_seed(9)
    for dtype in (torch.float32, torch.bfloat16):
        res = [torch.randn(M, C, device=dev()).to(dtype)]
        ys = [torch.randn(M, C, device=dev()).to(dtype) for _ in range(n)]
        gs = [torch.randn(M, C, device=dev()).to(dtype) for _ in range(n)]
        scale = torch.full((n, B), 1.0 / 0.7, device=dev())
        a = _res_abi(res, ys, gs, scale, B, _drop(0.0), True)
        b = _res_abi(res, ys, gs, scale, B, None, True, plain=True)
        assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]))  # p == 0: the plain kernels
        r1, r2 = _res_abi(res, ys, gs, scale, B, _drop(0.3), True), _res_abi(res, ys, gs, scale, B, _drop(0.3), True)
        assert all(torch.equal(x, y) for x, y in zip(r1[0] + r1[1], r2[0] + r2[1]))
        off = torch.ones(1, dtype=torch.int64, device=dev())
        r3 = _res_abi(res, ys, gs, scale, B, _drop(0.3, SEED, off), True)
        r4 = _res_abi(res, ys, gs, scale, B, _drop(0.3, SEED + 1), True)
        assert all(torch.equal(x, y) for x, y in zip(r3[0] + r3[1], r4[0] + r4[1]))
        assert not torch.equal(r1[0][0], r3[0][0])


# ---- 3. the block against its nn.Dropout path ------------------------------------------------------------------------------------------
class _MaskDropout(torch.nn.Module):
    """stands where an nn.Dropout stood (same p, but not in training mode: the block's nn.Dropout path runs and calls it) and applies
    the generator's mask of the call site: ``plan`` holds one (seed, site) per call of the block's forward, tensors of a call arrive in
    the order shared, tasks"""

    def __init__(self, rate, n):
        super().__init__()
        self.p, self.rate, self.n, self.plan, self.calls = rate, rate, n, [], 0
        self.training = False

    def forward(self, x):
        seed, site = self.plan[self.calls // self.n]
        k = self.calls % self.n
        self.calls += 1
        C = x.shape[-1]
        keep = O.dropout_keep_mask_t(seed, site + STRIDE * k, x.numel() // C, C, self.rate, device=x.device).view(x.shape)
        return torch.where(keep, x / (1 - self.rate), torch.zeros((), dtype=x.dtype, device=x.device))


def _block(tasks, drop):
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerBlock
    mt = O.mtlora_config(tasks, r_shared=8, r_task=4, dropout=0.05)
    blk = SwinTransformerBlock(96, (14, 14), 3, window_size=7, shift_size=3, lora=bool(tasks), tasks=tasks or None, mtlora=mt, layer_idx=0,
                               drop=drop, drop_path=0.1)
    O.det_fill_(blk.named_parameters())
    return blk.to(dev()).train()


def _run_block(blk, x, dtype, tasks, tag):
    from mtlora_amd import functional as Fn
    torch.manual_seed(77)
    Fn.droppath_reset()
    xin = x.clone().requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
    with ctx:
        y, yt = blk(xin)[:2]
    outs = [y] + [yt[t] for t in tasks]
    loss = sum((o.float() * O.det_tensor(f"actdrop.{tag}.{i}", o.shape, 1.0).to(dev())).sum() for i, o in enumerate(outs))
    blk.zero_grad(set_to_none=True)
    loss.backward()
    grads = {n: q.grad.clone() for n, q in blk.named_parameters() if q.grad is not None}
    return [o.detach().clone() for o in outs], xin.grad.clone(), grads


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tasks", [[], ["semseg", "normals"]])
def test_block_matches_its_dropout_path_with_the_generators_masks(tasks, dtype, monkeypatch):
    """seed order of a block: qkv, proj, PROJECTION, fc1, HIDDEN, fc2, MLP OUTPUT"""
    from mtlora_amd import functional as Fn
    n, rate = 1 + len(tasks), 0.1
    x = O.det_tensor("actdrop.x", (2, 196, 96), 1.0).to(dev()).float()
    blk = _block(tasks, rate)
    seeds, orig = [], Fn.next_seed

    def recording():
        seeds.append(orig())
        return seeds[-1]

    monkeypatch.setattr(Fn, "next_seed", recording)
    new = _run_block(blk, x, dtype, tasks, "t")
    assert len(seeds) == 7, seeds
    # the same block on its nn.Dropout path: the linear layers get their seeds back, the dropout modules the sites' seeds
    feed = iter([seeds[0], seeds[1], seeds[3], seeds[5]])
    monkeypatch.setattr(Fn, "next_seed", lambda: next(feed))
    blk.attn.proj_drop = _MaskDropout(rate, n if blk.attn.proj.tasks else 1)
    blk.attn.proj_drop.plan = [(seeds[2], PROJ)]
    blk.mlp.drop = _MaskDropout(rate, n)
    blk.mlp.drop.plan = [(seeds[4], HIDDEN), (seeds[6], MLP_OUT)]
    old = _run_block(blk, x, dtype, tasks, "t")
    assert blk.mlp.drop.calls == 2 * n and blk.attn.proj_drop.calls == n
    for i, (a, b) in enumerate(zip(new[0], old[0])):
        check(a, b, dtype, f"out{i}")
    check(new[1], old[1], dtype, "dx")
    assert set(new[2]) == set(old[2]) and len(new[2]) > 8
    for name in new[2]:
        check(new[2][name], old[2][name], dtype, f"grad {name}")


# ---- 4. the ATen ops that must be gone -------------------------------------------------------------------------------------------------
def _ops(blk, x):
    from mtlora_amd import functional as Fn
    from torch.profiler import ProfilerActivity, profile
    names = []
    for step in range(2):  # (an announced step draws DropPath from the step's bulk draw; the first one records the plan)
        xin = x.clone().requires_grad_(True)
        Fn.droppath_begin_step(x.device)
        try:
            with profile(activities=[ProfilerActivity.CPU]) as prof:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y, yt = blk(xin)[:2]
                (y.float().sum() + sum(v.float().sum() for v in yt.values())).backward()
                torch.cuda.synchronize()
        finally:
            Fn.droppath_end_step()
        names = [e.name for e in prof.events() if e.name.startswith("aten::")]
    return names


def test_no_aten_dropout_or_gelu_at_drop_rate():
    from mtlora_amd import functional as Fn
    tasks = ["semseg", "normals"]
    x = O.det_tensor("actdrop.x", (2, 196, 96), 1.0).to(dev()).float()
    Fn.droppath_reset()
    names = _ops(_block(tasks, 0.1), x)
    assert names
    for bad in ("aten::native_dropout", "aten::dropout", "aten::bernoulli_", "aten::gelu", "aten::gelu_backward"):
        assert bad not in names, bad
    # drop = 0: the op list does not depend on the dropout modules' mode -- nothing of the new paths runs
    Fn.droppath_reset()
    blk = _block(tasks, 0.0)
    a = _ops(blk, x)
    for m in (blk.mlp.drop, blk.attn.proj_drop, blk.attn.attn_drop):
        m.training = False
    Fn.droppath_reset()
    b = _ops(blk, x)
    assert a == b and "aten::native_dropout" not in a


# ---- 5. graph replay ---------------------------------------------------------------------------------------------------------------------
class _WeightedSum(torch.autograd.Function):
    """sum(x * w) without an ATen multi-block reduction (its memset does not replay: mtl_harness.GraphedTrainStep)"""

    @staticmethod
    def forward(ctx, x, w):
        from mtlora_amd import functional as Fn
        ctx.save_for_backward(w)
        ctx.dt = x.dtype
        return Fn.column_sum((x.float() * w).reshape(-1, x.shape[-1])).sum()

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return (g * w).to(ctx.dt), None


def test_graphed_train_step_draws_fresh_masks_and_replays_the_eager_step():
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd import swin_transformer_mtlora as S
    tasks = ["semseg", "normals"]
    mt = H.mtlora_namespace(tasks, 8, 4, n_stages=2, dropout=0.05)
    torch.manual_seed(5)
    bb = S.SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                                 window_size=7, drop_rate=0.1, drop_path_rate=0.0, tasks=tasks, mtlora=mt)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = bb

        def forward(self, x):
            return self.backbone(x, return_stages=True)

    model = Model().to(dev()).train()
    img = O.det_tensor("actdrop.img", (2, 3, 56, 56), 1.0).to(dev())
    weights = {}

    def crit(stages, targets):
        loss = 0
        for i, (s, tl) in enumerate(stages):
            for j, v in enumerate([s] + [tl[t] for t in tasks]):
                if (i, j) not in weights:
                    weights[(i, j)] = O.det_tensor(f"actdrop.w.{i}.{j}", v.shape, 1.0).to(dev())
                loss = loss + _WeightedSum.apply(v, weights[(i, j)])
        return loss, {}

    opt = H.build_optimizer(model, lr=0.0, capturable=True)
    drawn, orig = [0], Fn.next_seed

    def counting():
        drawn[0] += 1
        return orig()

    Fn.next_seed = counting
    try:
        warmup = 2
        gs = H.GraphedTrainStep(model, crit, opt, img, {}, clip_grad=5.0, warmup=warmup, fused_loss=False)
        assert gs.graphed, gs.why
        per_step = drawn[0] // (warmup + 1)
        assert per_step * (warmup + 1) == drawn[0] and per_step > 4 * 7
        losses = [gs().clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in losses)
        assert losses[0].item() != losses[1].item()  # lr = 0: the parameters stand still, the masks moved
        # the eager step with the host seeds of the captured step and the offset of the second replay
        Fn._seed_counter -= per_step
        gs.seed.sub_(gs.SEED_STEP)
        eager = gs._eager()
        torch.cuda.synchronize()
        assert torch.equal(eager, losses[1]), (eager.item(), losses[1].item())
    finally:
        Fn.next_seed = orig
        Fn.set_seed_offset(None)
