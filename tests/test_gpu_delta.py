"""Rank-aware dense update on the HIP path (csrc/delta.h): mtlora_delta_fwd / _bwd against fp64, and what is built on them."""
import ctypes

import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# one tile and step | partial tile in K, r tail, unaligned B rows | partial tile in N, unequal ranks | the target shape
SHAPES = [(32, 32, (8,)), (96, 40, (33,)), (40, 96, (100, 8, 33)), (288, 96, (256, 256, 256))]
EPS = 2.0 ** -24


def _call(fn, N, K, As, Bs, scale, sdev, *lists):
    from mtlora_amd import _lib as L
    n = len(As)
    st = getattr(L.lib(), fn)(n, N, K, (ctypes.c_int32 * n)(*[a.shape[0] for a in As]), L.ptr_array9(As), L.ptr_array9(Bs),
                              (ctypes.c_float * n)(*scale), L.ptr_array9(sdev), *[L.ptr_array9(p) for p in lists], L.stream_ptr())
    assert st == 0, (fn, st)


def _inputs(N, K, rs):
    g = torch.Generator().manual_seed(N * 1000 + K)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return [mk(r, K) for r in rs], [mk(N, r) for r in rs], [mk(N, K) for _ in rs]


@pytest.mark.parametrize("scales", ["host", "dev", "both"])
@pytest.mark.parametrize("N,K,rs", SHAPES)
def test_kernels_against_fp64(N, K, rs, scales):
    """every element of Delta W, dA and dB within the fp32 dot-product bound (n_red + 4) 2^-24 |s| (|.| |.|), evaluated in fp64"""
    As, Bs, Zs = _inputs(N, K, rs)
    n = len(rs)
    host = [1.0] * n if scales == "dev" else [0.5 * (i + 1) for i in range(n)]          # (products exact in fp32)
    dev = None if scales == "host" else [torch.tensor([-1.5 + i], device=DEV) for i in range(n)]
    out, dA, dB = [torch.empty(N, K, device=DEV) for _ in rs], [torch.empty_like(a) for a in As], [torch.empty_like(b) for b in Bs]
    _call("mtlora_delta_fwd", N, K, As, Bs, host, dev, out)
    _call("mtlora_delta_bwd", N, K, As, Bs, host, dev, Zs, dA, dB)
    for i in range(n):
        s = host[i] * (dev[i].item() if dev else 1.0)
        a, b, z = As[i].double(), Bs[i].double(), Zs[i].double()
        for what, got, ref, mag, n_red in (("dW", out[i], b @ a, b.abs() @ a.abs(), rs[i]), ("dA", dA[i], b.t() @ z, b.abs().t() @ z.abs(), N),
                                           ("dB", dB[i], z @ a.t(), z.abs() @ a.abs().t(), K)):
            err, bound = (got.double() - s * ref).abs(), (n_red + 4) * EPS * abs(s) * mag
            assert bool((err <= bound).all()), (what, i, (err / bound).max().item())


def test_null_outputs_guards_and_reproducibility():
    """a null dA[0] and dB[1] leave the other outputs bit-equal to the full call's; guards intact; two calls agree bit for bit"""
    N, K, rs = SHAPES[2]
    As, Bs, Zs = _inputs(N, K, rs)
    G = 4  # guard floats on either side (the outputs stay on 16 bytes)

    def run(skip_dA=(), skip_dB=()):
        bufs = [[torch.full((t.numel() + 2 * G,), 12345.0, device=DEV) for t in ts] for ts in (As, Bs)]
        ptrs = [[None if i in skip else b[G:] for i, b in enumerate(bs)] for bs, skip in zip(bufs, (skip_dA, skip_dB))]
        _call("mtlora_delta_bwd", N, K, As, Bs, [2.0] * len(rs), None, Zs, *ptrs)
        return bufs

    full, again, part = run(), run(), run(skip_dA=(0,), skip_dB=(1,))
    for kind in range(2):
        for i, (f, a, p) in enumerate(zip(full[kind], again[kind], part[kind])):
            assert torch.equal(f, a) and bool((f[:G] == 12345.0).all()) and bool((f[-G:] == 12345.0).all())
            assert not bool((f[G:-G] == 12345.0).any())
            skipped = i == (0, 1)[kind]
            assert bool((p == 12345.0).all()) if skipped else torch.equal(p, f), (kind, i)


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("use_xt", [True, False])
def test_layer_mixed_ranks_vs_fp64(use_xt, monkeypatch):
    """shared and task "a" rank-aware (128 > 96), task "b" low-rank: outputs, dx and factor gradients against the fp64 low-rank formula
    (reference lora.py:253-284) at the fp32 tolerance of test_linear_rank_aware_association_vs_oracle; ONE DeltaFn call"""
    from mtlora_amd import functional as Fn, lora
    from mtlora_amd.lora import MTLoRALinear
    monkeypatch.setattr(lora, "DELTA_HIP", True)
    tasks, M = ["a", "b"], 64
    torch.manual_seed(5)
    m = MTLoRALinear(96, 288, r={"shared": 128, "a": 128, "b": 8}, lora_shared_scale=2.0, lora_task_scale={"a": 1.5, "b": 1.5},
                     lora_dropout=0.0, tasks=tasks).to(DEV)
    with torch.no_grad():
        for n_, q in m.named_parameters():
            q.copy_(torch.randn_like(q) * (0.05 if "lora" in n_ else 0.02))
    m.linear.requires_grad_(False)
    calls, orig = [], Fn.DeltaFn.apply
    monkeypatch.setattr(Fn.DeltaFn, "apply", lambda n, *a: calls.append(n) or orig(n, *a))
    xs = [(0.5 * torch.randn(M, 96, device=DEV)).requires_grad_(True) for _ in range(3 if use_xt else 1)]
    y, yt = m(xs[0], {t: xs[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
    assert calls == [2], calls
    outs = [y] + [yt[t] for t in tasks]
    gys = [torch.randn(M, 288, device=DEV) for _ in outs]
    torch.autograd.backward(outs, gys)
    P = {k: v.detach().double().cpu().requires_grad_(v.requires_grad) for k, v in m.named_parameters()}
    xo = [x.detach().double().cpu().requires_grad_(True) for x in xs]
    yo, yto = O.mtlora_linear(xo[0], P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], 2.0, tasks=tasks,
                              A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                              scale_t=m.lora_task_scale, x_tasks={t: xo[1 + i] for i, t in enumerate(tasks)} if use_xt else None)
    refs = [yo] + [yto[t] for t in tasks]
    torch.autograd.backward(refs, [g.double().cpu() for g in gys])
    pairs = [(a, b.detach()) for a, b in zip(outs, refs)] + [(a.grad, b.grad) for a, b in zip(xs, xo)]
    pairs += [(q.grad, P[n_].grad) for n_, q in m.named_parameters() if q.requires_grad]
    for i, (a, b) in enumerate(pairs):
        assert _rel(a, b) <= 1e-3, (i, _rel(a, b))


def test_merge_with_a_trainable_scale_is_capturable():
    """merge() with a trainable shared scale makes no host read: it can be captured; the replayed merge gives the unmerged output
    (tolerance of test_merge_matches_unmerged_eval), and unmerge() restores W + d - d bit for bit"""
    from mtlora_amd.lora import MTLoRALinear
    torch.manual_seed(6)
    m = MTLoRALinear(96, 192, r=16, lora_shared_scale=2.0, tasks=None, trainable_scale_shared=True).to(DEV)
    with torch.no_grad():
        m.lora_shared_B.normal_(0.0, 0.05)
    m.eval()
    x = torch.randn(50, 96, device=DEV)
    with torch.no_grad():
        ref = m(x)[0].clone()
        w0, d = m.linear.weight.detach().clone(), m._shared_delta()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert m.merge()
        m.linear.weight.copy_(w0)  # (whether or not capturing ran the add: the replay does)
        graph.replay()
        assert torch.equal(m.linear.weight, w0 + d)
        assert _rel(m(x)[0], ref) <= 1e-3
        assert m.unmerge() and torch.equal(m.linear.weight, w0 + d - d)


def test_graphed_train_step_with_rank_aware_layers(monkeypatch):
    """a 2-block model with rank-aware stage-0 layers (128 > 96): 3 replays against 3 eager steps under the criterion of
    test_gpu_optim_capturable.test_whole_step_graphed_with_scaler (losses within 2e-3, cosine of the updates >= 0.98)"""
    from mtlora_amd import functional as Fn, lora
    from mtlora_amd import mtl_harness as H
    monkeypatch.setattr(lora, "DELTA_HIP", True)
    tasks = ["semseg", "normals"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=17, device=DEV)
    out = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(img_size=224, tasks=tasks, depths=(1, 1), num_heads=(3, 6), r_shared=128, drop_path_rate=0.0, seed=4).to(DEV).train()
        assert any(l.rank_aware_shared() for l in model.modules() if hasattr(l, "rank_aware_shared"))
        crit, opt = H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2)
            assert gs.graphed is True and gs.why == "", gs.why
            drawn = Fn._seed_counter
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses = []
            for _ in range(3):
                if not use_graph:  # the eager step, drawing the seeds the capture drew and walking the same device offset
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                losses.append((gs() if use_graph else H.train_step(model, crit, opt, img, tg, clip_grad=5.0)[0]).item())
            out.append((losses, {n: (p.detach() - start[n]).double() for n, p in model.named_parameters() if n in start}))
        finally:
            Fn.set_seed_offset(None)
    for a, b in zip(out[0][0], out[1][0]):
        assert abs(a - b) <= 2e-3 * abs(b), (a, b)
    dot = lambda u, v: sum((u[n] * v[n]).sum().item() for n in u)
    cos = dot(out[0][1], out[1][1]) / (dot(out[0][1], out[0][1]) * dot(out[1][1], out[1][1])) ** 0.5
    assert cos >= 0.98, cos
