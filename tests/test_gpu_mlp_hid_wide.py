"""The task-enabled Mlp with implicit task hidden tensors at task ranks 16 .. 128 (csrc/hid_wide.h, ``Fn.set_mlp_hid_wide``) against the
fp64 formulas of the reference (lora.py:253-284 applied twice with GELU between)."""
import pytest
import torch

from test_gpu_kernels import _log_parity, assert_close, dev, rel_err

pytestmark = pytest.mark.gpu

# name: (M, C, hidden, fc1 task ranks, fc2 task ranks)
GEOM = {"a": (77, 32, 128, (16,), (16,)),                       # row tail, one column chunk
        "b": (200, 64, 384, (16, 48, 32), (32, 16, 16)),        # three chunks, half-filled rank tiles, ranks that differ by task and layer
        "c": (130, 128, 256, (128, 128), (128, 128))}           # four rank tiles / eight k steps
# case: (geometry, max_cu, outputs WITHOUT a gradient)
CASES = {"a": ("a", 0, ()), "b": ("b", 0, ()), "c": ("c", 0, ()),
         "d-persist": ("b", 1, ()),                             # one workgroup walks every row block; the partial reduce has one term
         "e-miss1": ("b", 0, (2,)), "e-missall": ("b", 0, (1, 2, 3))}


def _mlp(tasks, C, Hd, r1, r2):
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.swin_transformer_mtlora import Mlp
    torch.manual_seed(31)
    mk = lambda r: Mlp(C, Hd, lora=True, tasks=tasks, layer_idx=0, mtlora=H.mtlora_namespace(
        tasks, scale=2.0, dropout=0.0, R_PER_TASK_LIST=[{"shared": 16, **dict(zip(tasks, r))}] * 4))
    mlp = mk(r1)
    mlp.fc2 = mk(r2).fc2
    mlp = mlp.to(dev())
    with torch.no_grad():
        for n_, p_ in mlp.named_parameters():
            if "lora_" in n_:
                p_.normal_(0, 0.1)
            else:
                p_.requires_grad_(False)
    return mlp.train()


def _reference(mlp, xs, tasks, live, gys):
    P = {n: p.detach().double().requires_grad_(p.requires_grad) for n, p in mlp.named_parameters()}
    X = [x.detach().double().requires_grad_(True) for x in xs]

    def lin(pre, x, xt):
        base = x @ P[f"{pre}.linear.weight"].t() + P[f"{pre}.linear.bias"]
        m = getattr(mlp, pre)
        ys = base + float(m.lora_shared_scale) * (x @ P[f"{pre}.lora_shared_A"].t()) @ P[f"{pre}.lora_shared_B"].t()
        return ys, [base + float(m.lora_task_scale[t]) * (v @ P[f"{pre}.lora_tasks_A.{t}"].t()) @ P[f"{pre}.lora_tasks_B.{t}"].t()
                    for v, t in zip(xt, tasks)]
    g = torch.nn.functional.gelu
    h, ht = lin("fc1", X[0], X[1:])
    y, yt = lin("fc2", g(h), [g(v) for v in ht])
    outs = [y] + yt
    torch.autograd.backward([outs[i] for i in live], [gys[i].double() for i in live])
    return outs, [x.grad for x in X], {n: p.grad for n, p in P.items() if p.grad is not None}


def _run(mlp, xs, tasks, live, gys, dtype, hid, wide):
    from mtlora_amd import functional as Fn
    old = Fn.set_mlp_hid(hid), Fn.set_mlp_hid_wide(wide)
    try:
        for x in xs:
            x.grad = None
        mlp.zero_grad()
        with torch.autocast("cuda", dtype=dtype):
            y, y_t = mlp(xs[0], dict(zip(tasks, xs[1:])))
        outs = [y] + [y_t[t] for t in tasks]
        torch.autograd.backward([outs[i] for i in live], [gys[i] for i in live])
        return ([o.detach().clone() for o in outs], [None if x.grad is None else x.grad.clone() for x in xs],
                {n: p.grad.clone() for n, p in mlp.named_parameters() if p.grad is not None})
    finally:
        Fn.set_mlp_hid(old[0])
        Fn.set_mlp_hid_wide(old[1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", list(CASES))
def test_mlp_hid_wide_vs_fp64(case, dtype):
    from mtlora_amd import functional as Fn
    geom, max_cu, missing = CASES[case]
    M, C, Hd, r1, r2 = GEOM[geom]
    tasks = [f"t{i}" for i in range(len(r1))]
    mlp = _mlp(tasks, C, Hd, r1, r2)
    assert Fn.mlp_hidr_supported(mlp.fc1.hid_call(dtype, dev())[0], mlp.fc2.hid_call(dtype, dev())[0], M)
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randn(M, C, device=dev(), generator=g).to(dtype).float().requires_grad_(True) for _ in range(1 + len(tasks))]
    gys = [torch.randn(M, C, device=dev(), generator=g).to(dtype) for _ in range(1 + len(tasks))]
    live = [i for i in range(1 + len(tasks)) if i not in missing]
    ro, rg, rp = _reference(mlp, xs, tasks, live, gys)
    prev = Fn.set_tuning(max_cu=max_cu)
    try:
        layer = _run(mlp, xs, tasks, live, gys, dtype, False, False)   # the per-layer path
        off = _run(mlp, xs, tasks, live, gys, dtype, True, False)      # default switches: routing unchanged
        on = _run(mlp, xs, tasks, live, gys, dtype, True, True)
        again = _run(mlp, xs, tasks, live, gys, dtype, True, True)
    finally:
        Fn.set_tuning(**prev)
    for a, b in zip(layer[0] + layer[1], off[0] + off[1]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert layer[2].keys() == off[2].keys() and all(torch.equal(layer[2][k], off[2][k]) for k in off[2])
    for a, b in zip(on[1], again[1]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert on[2].keys() == again[2].keys() == rp.keys() and all(torch.equal(on[2][k], again[2][k]) for k in rp)

    def check(what, got, old, ref):
        if ref is None:  # no gradient reaches this tensor: none, or zeros
            assert got is None or not got.any(), what
            return
        _log_parity(f"hid wide {case} {what}: per-layer path", rel_err(old, ref), 0.0, 1.0)
        assert_close(got, ref, dtype, f"hid wide {case} {what}")
    for i in range(1 + len(tasks)):
        check(f"y{i}", on[0][i], layer[0][i], ro[i].detach())
        check(f"dx{i}", on[1][i], layer[1][i], rg[i])
    for k in rp:
        check(f"d{k}", on[2][k], layer[2][k], rp[k])
