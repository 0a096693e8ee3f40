"""SHARED_MODE "addition" on the HIP path: ``mtlora_sum_ln_add_fwd / _bwd`` (out = y + LayerNorm(sum_k y_t[k]), reference
lora.py:275-284) against the portable definition in fp64, their aliasing / determinism / argument / non-finite contracts, and the
layer, a small backbone and a captured graph that run through them.

Tolerances are those of tests/test_gpu_kernels.py, restated: max-norm relative error, 1e-3 fp32, 1e-2 bf16, 2e-3 fp16."""
import ctypes

import pytest
import torch

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2, torch.float16: 2e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EPS = 1e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def assert_close(a, b, dtype, what):
    e = rel_err(a, b)
    print(f"{what}: rel err {e:.3e} (tol {TOL[dtype]:.0e})")
    assert e <= TOL[dtype], f"{what}: rel err {e:.3e} > {TOL[dtype]:.1e}"


def make_inputs(M, N, n, dtype, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 * n + M + N + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    yts = [(r(M, N) * (0.5 + 0.25 * k) + 0.1 * k).to(dev()).to(dtype) for k in range(n)]
    y = r(M, N).to(dev()).to(dtype)
    w = (r(N) * 0.2 + 1).to(dev())
    b = (r(N) * 0.1).to(dev())
    dout = r(M, N).to(dev()).to(dtype)
    adds = [r(M, N).to(dev()).to(dtype) for _ in range(n)]
    return y, yts, w, b, dout, adds


def nan_rows(M, *rest, dtype=torch.float32):
    return torch.full((M, *rest), float("nan"), dtype=dtype, device=dev())


def nan_like(t):
    return nan_rows(*t.shape, dtype=t.dtype)


def k_fwd(y, yts, w, b, out=None, n=None, N=None):
    """(status, out, mean, rstd)"""
    from mtlora_amd import _lib as L
    M, Nn = y.shape
    out = nan_like(y) if out is None else out
    mean, rstd = nan_rows(M), nan_rows(M)
    st = L.lib().mtlora_sum_ln_add_fwd(len(yts) if n is None else n, L.ptr_array(yts), L.ptr(y), L.ptr(w), L.ptr(b), L.ptr(out),
                                              L.ptr(mean), L.ptr(rstd), M, Nn if N is None else N, EPS, L.dtype_code(y), L.stream_ptr())
    return st, out, mean, rstd


def k_bwd(dout, yts, w, mean, rstd, adds, dys=None, n=None, N=None, scratch_bytes=None):
    """(status, dys, dgamma, dbeta)"""
    from mtlora_amd import _lib as L
    lib = L.lib()
    M, Nn = dout.shape
    code = L.dtype_code(dout)
    sb = lib.mtlora_sum_ln_add_bwd_scratch_bytes(len(yts), M, Nn, code)
    assert sb > 0
    scratch = torch.empty(sb, dtype=torch.uint8, device=dout.device)
    dys = [nan_like(dout) for _ in yts] if dys is None else dys
    dg = torch.full((Nn,), float("nan"), device=dout.device)
    db = torch.full((Nn,), float("nan"), device=dout.device)
    st = lib.mtlora_sum_ln_add_bwd(len(yts) if n is None else n, L.ptr(dout), L.ptr_array(yts), L.ptr(w), L.ptr(mean), L.ptr(rstd),
                                          L.ptr_array(adds) if adds is not None else None, L.ptr_array(dys), L.ptr(dg), L.ptr(db), M,
                                          Nn if N is None else N, code, L.ptr(scratch), sb if scratch_bytes is None else scratch_bytes,
                                          L.stream_ptr())
    return st, dys, dg, db


# (M, N, n): single row / narrowest width / one task; the fixture's task count at the narrowest Swin width; M off every row-tile
# boundary; the widest Swin-T row; Swin-B width with the maximum task count; empty
SHAPES = [(1, 96, 1), (98, 96, 4), (131, 288, 3), (70, 3072, 4), (33, 4096, 8), (0, 96, 2)]


@pytest.mark.parametrize("addends", ["all", "some", "none"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_fp64(shape, dtype, addends):
    from mtlora_amd import functional as Fn
    M, N, n = shape
    y, yts, w, b, dout, adds = make_inputs(M, N, n, dtype)
    if addends == "some":
        adds = [a if k % 2 == 0 else None for k, a in enumerate(adds)]
        if n == 1:
            adds = [None]
    st, out, mean, rstd = k_fwd(y, yts, w, b)
    assert st == 0
    st, dys, dg, db = k_bwd(dout, yts, w, mean, rstd, None if addends == "none" else adds)
    assert st == 0
    torch.cuda.synchronize()
    if M == 0:
        assert torch.equal(dg, torch.zeros_like(dg)) and torch.equal(db, torch.zeros_like(db))
        return
    y64 = y.double().requires_grad_(True)
    yt64 = [t.double().requires_grad_(True) for t in yts]
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = Fn.sum_norm_add_torch(y64, yt64, w64, b64, EPS)
    loss = (ref * dout.double()).sum()
    if addends != "none":
        for t, a in zip(yt64, adds):
            if a is not None:
                loss = loss + (t * a.double()).sum()
    loss.backward()
    assert_close(out, ref, dtype, "out")
    for k in range(n):
        assert_close(dys[k], yt64[k].grad, dtype, f"dy_t[{k}]")
    assert_close(dg, w64.grad, dtype, "dgamma")
    assert_close(db, b64.grad, dtype, "dbeta")
    assert torch.equal(y64.grad, dout.double())  # the gradient of y is dout itself: the kernel writes nothing for it


@pytest.mark.parametrize("dtype", DTYPES)
def test_aliasing_and_determinism(dtype):
    M, N, n = 131, 288, 3
    y, yts, w, b, dout, adds = make_inputs(M, N, n, dtype, seed=1)
    st, out, mean, rstd = k_fwd(y, yts, w, b)
    assert st == 0
    y_alias = y.clone()
    st, out2, mean2, rstd2 = k_fwd(y_alias, yts, w, b, out=y_alias)
    assert st == 0 and out2.data_ptr() == y_alias.data_ptr()
    assert torch.equal(out, out2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    st, dys, dg, db = k_bwd(dout, yts, w, mean, rstd, adds)
    assert st == 0
    alias = [a.clone() for a in adds]
    st, dys2, dg2, db2 = k_bwd(dout, yts, w, mean, rstd, alias, dys=alias)
    assert st == 0
    torch.cuda.synchronize()
    for k in range(n):
        assert torch.equal(dys[k], dys2[k]), k
        assert not torch.isnan(dys[k].float()).any()
    assert torch.equal(dg, dg2) and torch.equal(db, db2)  # two calls on the same inputs: bit-equal parameter gradients
    assert not torch.isnan(dg).any() and not torch.isnan(db).any()


def test_argument_errors_launch_nothing():
    from mtlora_amd import _lib as L
    lib = L.lib()
    M, N, n = 12, 96, 2
    y, yts, w, b, dout, adds = make_inputs(M, N, n, torch.bfloat16)
    st, out, mean, rstd = k_fwd(y, yts, w, b)
    assert st == 0
    torch.cuda.synchronize()
    L.check(lib.mtlora_prof_begin(64), "prof_begin")
    sentinel = torch.full_like(y, 7.0)
    codes = {
        "fwd n=0": k_fwd(y, yts, w, b, out=sentinel, n=0)[0],
        "fwd n=9": k_fwd(y, yts, w, b, out=sentinel, n=9)[0],
        "fwd N=100": k_fwd(y, yts, w, b, out=sentinel, N=100)[0],
        "fwd null y_t[1]": k_fwd(y, [yts[0], None], w, b, out=sentinel, n=2)[0],
    }
    dsent = [torch.full_like(y, 7.0) for _ in range(n)]
    codes.update({
        "bwd n=0": k_bwd(dout, yts, w, mean, rstd, adds, dys=dsent, n=0)[0],
        "bwd n=9": k_bwd(dout, yts, w, mean, rstd, adds, dys=dsent, n=9)[0],
        "bwd N=100": k_bwd(dout, yts, w, mean, rstd, adds, dys=dsent, N=100)[0],
        "bwd null y_t[1]": k_bwd(dout, [yts[0], None], w, mean, rstd, adds, dys=dsent, n=2)[0],
        "bwd short scratch": k_bwd(dout, yts, w, mean, rstd, adds, dys=dsent, scratch_bytes=64)[0],
    })
    s = L.ProfSummary()
    L.check(lib.mtlora_prof_end(ctypes.byref(s)), "prof_end")
    torch.cuda.synchronize()
    for what, code in codes.items():
        assert code < 0, (what, code)
    assert sum(s.count[k] for k in range(L.PROF_KINDS)) == 0
    assert torch.equal(sentinel, torch.full_like(y, 7.0)) and all(torch.equal(d, torch.full_like(y, 7.0)) for d in dsent)
    assert lib.mtlora_sum_ln_add_bwd_scratch_bytes(9, M, N, L.BF16) == -1
    assert lib.mtlora_sum_ln_add_bwd_scratch_bytes(2, M, 100, L.BF16) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_poisons_its_row_only(dtype):
    M, N, n = 37, 96, 3
    y, yts, w, b, dout, adds = make_inputs(M, N, n, dtype, seed=2)
    st, out, mean, rstd = k_fwd(y, yts, w, b)
    st2, dys, dg, db = k_bwd(dout, yts, w, mean, rstd, adds)
    bad = [t.clone() for t in yts]
    bad[1][5, 17] = float("nan")
    st3, out_b, mean_b, rstd_b = k_fwd(y, bad, w, b)
    st4, dys_b, dg_b, db_b = k_bwd(dout, bad, w, mean_b, rstd_b, adds)
    assert st == st2 == st3 == st4 == 0
    torch.cuda.synchronize()
    keep = torch.ones(M, dtype=torch.bool, device=dev())
    keep[5] = False
    assert torch.isnan(out_b[5].float()).all() and torch.equal(out_b[keep], out[keep])
    for k in range(n):
        assert torch.isnan(dys_b[k][5].float()).all(), k
        assert torch.equal(dys_b[k][keep], dys[k][keep]), k
    assert torch.isnan(dg_b).all()  # every column's dgamma sums row 5
    assert torch.equal(db_b, db)    # dbeta sums dout only


# ------------------------------------------------------------------------------------------------
# the layer
# ------------------------------------------------------------------------------------------------
def build_layer(c):
    from mtlora_amd.lora import MTLoRALinear
    N, K = c["params"]["linear.weight"].shape
    m = MTLoRALinear(K, N, r=c["r"], lora_shared_scale=c["scale_s"], lora_task_scale=c["scale_t"], lora_dropout=0.0, tasks=c["tasks"],
                     shared_mode=c["mode"], bias=c["bias"])
    m.load_state_dict({k: v.float() for k, v in c["params"].items()})
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    return m.to(dev())


def run_layer(m, c, dtype):
    x = c["x"].to(dev()).float().requires_grad_(True)
    xt = {t: v.to(dev()).float().requires_grad_(True) for t, v in c["x_tasks"].items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        y, yt = m(x, xt)
    loss = (y.float() * c["gy"].to(dev()).float()).sum()
    for t in c["tasks"]:
        loss = loss + (yt[t].float() * c["gy_tasks"][t].to(dev()).float()).sum()
    loss.backward()
    return x, xt, y, yt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layer_against_the_golden_fixture(golden, dtype):
    c = golden("linear.pt")["addition_xtasks"]
    m = build_layer(c)
    x, xt, y, yt = run_layer(m, c, dtype)
    assert y.dtype == dtype
    assert_close(y, c["y"], dtype, "y")
    assert_close(x.grad, c["dx"], dtype, "dx")
    for t in c["tasks"]:
        assert_close(yt[t], c["y_tasks"][t], dtype, f"y[{t}]")
        assert_close(xt[t].grad, c["dx_tasks"][t], dtype, f"dx[{t}]")
    named = dict(m.named_parameters())
    seen = set()
    for n, g in c["grads"].items():
        if n.startswith("linear."):
            continue
        assert_close(named[n].grad, g, dtype, f"grad {n}")
        seen.add(n)
    assert {"lora_norm.weight", "lora_norm.bias"} <= seen


def test_the_fused_path_is_taken(golden, monkeypatch):
    """forward + backward of the layer complete with the ATen pieces of the old form made to raise, and the launch records hold the
    new kinds once per direction"""
    from mtlora_amd import _lib as L
    lib = L.lib()
    c = golden("linear.pt")["addition_xtasks"]
    m = build_layer(c)

    def refuse(*a, **k):
        raise AssertionError("the ATen form of shared_mode='addition' ran")

    monkeypatch.setattr(torch.nn.functional, "layer_norm", refuse)
    monkeypatch.setattr(torch, "stack", refuse)
    L.check(lib.mtlora_prof_begin(256), "prof_begin")
    x, xt, y, yt = run_layer(m, c, torch.float32)
    s = L.ProfSummary()
    L.check(lib.mtlora_prof_end(ctypes.byref(s)), "prof_end")
    monkeypatch.undo()
    names = {lib.mtlora_prof_kind_name(k).decode(): s.count[k] for k in range(L.PROF_KINDS) if s.count[k]}
    assert names.get("k_sum_ln_add_fwd") == 1 and names.get("k_sum_ln_add_bwd") == 1, names
    assert_close(y, c["y"], torch.float32, "y")
    assert m.lora_norm.weight.grad is not None and m.lora_norm.bias.grad is not None


def test_frozen_lora_norm_gets_no_gradient(golden):
    c = golden("linear.pt")["addition_xtasks"]
    m = build_layer(c)
    m.lora_norm.weight.requires_grad_(False)
    m.lora_norm.bias.requires_grad_(False)
    x, xt, y, yt = run_layer(m, c, torch.float32)
    assert m.lora_norm.weight.grad is None and m.lora_norm.bias.grad is None
    assert_close(x.grad, c["dx"], torch.float32, "dx")
    for t in c["tasks"]:
        assert_close(xt[t].grad, c["dx_tasks"][t], torch.float32, f"dx[{t}]")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_layer_replays_bit_exact(dtype):
    from mtlora_amd.lora import MTLoRALinear
    K, N, M, tasks = 96, 384, 300, ["a", "b", "c"]
    torch.manual_seed(5)
    m = MTLoRALinear(K, N, r={"shared": 16, **{t: 4 for t in tasks}}, lora_shared_scale=2.0, lora_task_scale={t: 3.0 for t in tasks},
                     lora_dropout=0.0, tasks=tasks, shared_mode="addition").to(dev()).eval()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            p.copy_(torch.randn_like(p) * 0.05 + (1.0 if n_ == "lora_norm.weight" else 0.0))
    m.linear.weight.requires_grad_(False)
    m.linear.bias.requires_grad_(False)
    params = [q for q in m.parameters() if q.requires_grad]
    xs = torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True)
    xts = {t: torch.randn(M, K, device=dev()).to(dtype).requires_grad_(True) for t in tasks}
    gy = [torch.randn(M, N, device=dev()).to(dtype) for _ in range(1 + len(tasks))]

    def step():
        y, yt = m(xs, xts)
        loss = (y.float() * gy[0].float()).sum()
        for i, t in enumerate(tasks):
            loss = loss + (yt[t].float() * gy[1 + i].float()).sum()
        grads = torch.autograd.grad(loss, [xs, *xts.values(), *params])
        return [y, *yt.values(), *grads]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    for k in range(2):
        with torch.no_grad():
            xs.copy_(torch.randn(M, K, device=dev()).to(dtype))
            for t in tasks:
                xts[t].copy_(torch.randn(M, K, device=dev()).to(dtype))
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        want = step()
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (k, i)


# ------------------------------------------------------------------------------------------------
# a 2-stage backbone with SHARED_MODE "addition" against the oracle in fp64
# ------------------------------------------------------------------------------------------------
def _sampled(P, stages, tasks, tag):
    loss = 0
    for i, (st, tl) in enumerate(stages):
        loss = loss + (st.double() * O.det_tensor(f"{tag}.g.{i}", st.shape, 1.0).to(st.device).double()).sum()
        for t in tasks:
            loss = loss + (tl[t].double() * O.det_tensor(f"{tag}.g.{i}.{t}", st.shape, 1.0).to(st.device).double()).sum()
    return loss


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_backbone_against_the_oracle(dtype):
    from mtlora_amd.lora import mark_only_lora_as_trainable
    from mtlora_amd.swin_transformer_mtlora import SwinTransformerMTLoRA
    tasks = ["semseg", "normals"]
    cfg = O.swin_t_cfg(img_size=56, tasks=tasks, r_shared=8, r_task=4, depths=(2, 2), num_heads=(3, 6), drop_path_rate=0.1,
                       dropout=0.05, shared_mode="addition")
    bb = SwinTransformerMTLoRA(img_size=56, patch_size=4, in_chans=3, num_classes=0, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                               window_size=7, drop_path_rate=0.1, tasks=tasks, mtlora=cfg["mtlora"])
    shapes = O.backbone_param_shapes(cfg)
    O.det_fill_(bb.named_parameters())
    mark_only_lora_as_trainable(bb, bias="none")
    norms = [n for n, p in bb.named_parameters() if "lora_norm" in n]
    assert len(norms) == 12 and all(dict(bb.named_parameters())[n].requires_grad for n in norms)  # 3 task-enabled layers x 2 stages
    bb = bb.to(dev()).eval()
    x = O.det_tensor("bba.x", (1, 3, 56, 56), 1.0)
    # reference: the oracle in fp64 on the host
    P = {k: v.requires_grad_(True) for k, v in O.make_params(shapes, torch.float64).items()}
    ref = O.backbone_stages(P, x.double(), cfg)
    _sampled(P, ref, tasks, "bba").backward()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        stages = bb(x.to(dev()), return_stages=True)
    for i, (s, tl) in enumerate(stages):
        assert_close(s, ref[i][0], dtype, f"stage {i}")
        for t in tasks:
            assert_close(tl[t], ref[i][1][t], dtype, f"stage {i} {t}")
    _sampled(None, [(s.float(), {t: v.float() for t, v in tl.items()}) for s, tl in stages], tasks, "bba").backward()
    # gradients: the tolerance + what the reference's own eager dataflow in this dtype (the oracle's ATen ops under the same autocast,
    # on this GPU) loses on that tensor against fp64, measured here; fp32: the tolerance alone
    eager = {}
    if dtype != torch.float32:
        Pe = {k: v.to(dev()).requires_grad_(True) for k, v in O.make_params(shapes).items()}
        with torch.autocast("cuda", dtype=dtype):
            es = O.backbone_stages(Pe, x.to(dev()), cfg)
        _sampled(Pe, [(s.float(), {t: v.float() for t, v in tl.items()}) for s, tl in es], tasks, "bba").backward()
        eager = {n: rel_err(Pe[n].grad, P[n].grad) for n in shapes if Pe[n].grad is not None and P[n].grad is not None}
    named = dict(bb.named_parameters())
    factors = [f"layers.{i}.blocks.1.mlp.fc1.lora_tasks_B.{tasks[0]}" for i in range(2)]
    assert set(norms + factors) <= set(shapes)
    for n in norms + factors:
        e = rel_err(named[n].grad, P[n].grad)
        gate = TOL[dtype] + eager.get(n, 0.0)
        print(f"grad {n}: rel err {e:.3e} (gate {gate:.3e}, eager {eager.get(n, 0.0):.3e})")
        assert e <= gate, (n, e, gate)
