"""SHARED_MODE "addition" without a GPU: the portable definition ``functional.sum_norm_add_torch`` against the fixture captured from
the reference (tests/golden/linear.pt, case ``addition_xtasks``) and against the fp64 oracle, the three new C-ABI symbols, and the
unchanged ATen form of an ``addition`` MTLoRALinear off the device."""
import os
import re

import torch

from oracle import mtlora_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtlora_sum_ln_add_fwd", "mtlora_sum_ln_add_bwd_scratch_bytes", "mtlora_sum_ln_add_bwd")


def _case(golden):
    c = golden("linear.pt")["addition_xtasks"]
    assert c["mode"] == "addition"
    return c


def _pretrained(c):
    """x W^T + b of the fixture: what the layer adds the normalised sum to"""
    return torch.nn.functional.linear(c["x"], c["params"]["linear.weight"], c["params"]["linear.bias"])


def test_sum_norm_add_torch_reproduces_the_fixture(golden):
    from mtlora_amd import functional as Fn
    c = _case(golden)
    yt = [c["y_tasks"][t].float() for t in c["tasks"]]
    got = Fn.sum_norm_add_torch(_pretrained(c).float(), yt, c["params"]["lora_norm.weight"].float(), c["params"]["lora_norm.bias"].float(),
                                1e-5)
    assert got.dtype == torch.float32
    err = ((got.double() - c["y"]).abs().max() / c["y"].abs().max()).item()
    assert err <= 1e-6, err


def test_sum_norm_add_torch_gradients_match_the_oracle(golden):
    from mtlora_amd import functional as Fn
    c = _case(golden)
    tasks = c["tasks"]
    P = {k: v.double().clone().requires_grad_(True) for k, v in c["params"].items()}
    x = c["x"].double().clone().requires_grad_(True)
    xt = {t: c["x_tasks"][t].double().clone().requires_grad_(True) for t in tasks}
    y, yt = O.mtlora_linear(x, P["linear.weight"], P["linear.bias"], None, None, 0.0, tasks=tasks,
                            A_t={t: P["lora_tasks_A." + t] for t in tasks}, B_t={t: P["lora_tasks_B." + t] for t in tasks},
                            scale_t=c["scale_t"], x_tasks=xt, shared_mode="addition",
                            lora_norm=(P["lora_norm.weight"], P["lora_norm.bias"]))
    # the oracle's own parts, detached, through the portable definition
    y0 = torch.nn.functional.linear(x.detach(), P["linear.weight"].detach(), P["linear.bias"].detach()).requires_grad_(True)
    ys = [yt[t].detach().clone().requires_grad_(True) for t in tasks]
    w, b = P["lora_norm.weight"].detach().clone().requires_grad_(True), P["lora_norm.bias"].detach().clone().requires_grad_(True)
    out = Fn.sum_norm_add_torch(y0, ys, w, b, 1e-5)
    assert out.dtype == torch.float64
    assert torch.allclose(out, y, rtol=0, atol=1e-12)
    gy = c["gy"].double()
    (out * gy).sum().backward()
    want = torch.autograd.grad((y * gy).sum(), [P["lora_norm.weight"], P["lora_norm.bias"]] + [yt[t] for t in tasks])
    for got, ref, what in zip([w.grad, b.grad] + [t.grad for t in ys], want, ["dgamma", "dbeta"] + tasks):
        assert ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item() <= 1e-10, what
    assert torch.equal(y0.grad, gy)  # the gradient of the pretrained output is the incoming one


def test_new_symbols_declared_and_bound():
    from mtlora_amd import _lib
    header = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+MTLORA_ABI_VERSION\s+12\b", header) and _lib.ABI_VERSION == 12
    assert "lora.py:275-284" in header


def test_host_rejects_every_single_defect():
    """the return code of both launch entries for calls with ONE defect each, all rejected on the host (pointers are fake addresses that
    are never dereferenced: no row may reach a launch), and the calls without rows, which return OK before any pointer is looked at"""
    import ctypes
    from mtlora_amd import _lib as L
    lib = L.lib()
    OK, DTYPE, SHAPE, ALIGN, NULL, WORK, UNSUP = 0, -1, -2, -3, -4, -5, -7
    P = lambda j: ctypes.c_void_p(4096 * (j + 1))

    def arr(j, n=3, null=None, odd=None):
        a = L.PtrArr()
        for k in range(n):
            a[k] = 4096 * (j + 1) + 64 * k
        if null is not None:
            a[null] = None
        if odd is not None:
            a[odd] = 4096 * (j + 1) + 64 * odd + 4
        return a

    good = dict(n=3, y_t=arr(0), y=P(1), gamma=P(2), beta=P(3), out=P(4), mean=P(5), rstd=P(6), M=12, N=64, dtype=L.F32,
                dout=P(7), add=arr(8), dy_t=arr(9), dgamma=P(10), dbeta=P(11), scratch=P(12), scratch_bytes=1 << 40)

    def fwd(**e):
        a = {**good, **e}
        return lib.mtlora_sum_ln_add_fwd(a["n"], a["y_t"], a["y"], a["gamma"], a["beta"], a["out"], a["mean"], a["rstd"], a["M"], a["N"],
                                         1e-5, a["dtype"], None)

    def bwd(**e):
        a = {**good, **e}
        return lib.mtlora_sum_ln_add_bwd(a["n"], a["dout"], a["y_t"], a["gamma"], a["mean"], a["rstd"], a["add"], a["dy_t"], a["dgamma"],
                                         a["dbeta"], a["M"], a["N"], a["dtype"], a["scratch"], a["scratch_bytes"], None)

    odd = lambda j: ctypes.c_void_p(4096 * (j + 1) + 4)
    both = [(DTYPE, dict(dtype=7)), (DTYPE, dict(dtype=-1)), (DTYPE, dict(dtype=L.U8)), (SHAPE, dict(N=66)), (SHAPE, dict(N=100, dtype=L.BF16)),
            (SHAPE, dict(N=0)), (SHAPE, dict(N=-64)), (SHAPE, dict(M=-1)), (UNSUP, dict(N=4100)), (UNSUP, dict(N=4104, dtype=L.BF16)),
            (UNSUP, dict(N=4104, dtype=L.F16)), (SHAPE, dict(n=0)), (SHAPE, dict(n=-1)), (SHAPE, dict(n=9)),
            (NULL, dict(y_t=None)), (NULL, dict(y_t=arr(0, null=0))), (NULL, dict(y_t=arr(0, null=2))), (NULL, dict(gamma=None)),
            (NULL, dict(mean=None)), (NULL, dict(rstd=None)), (ALIGN, dict(y_t=arr(0, odd=0))), (ALIGN, dict(y_t=arr(0, odd=2))),
            (ALIGN, dict(gamma=odd(2)))]
    for want, e in both:
        assert fwd(**e) == want, ("fwd", e)
        assert bwd(**e) == want, ("bwd", e)
    for want, e in [(NULL, dict(y=None)), (NULL, dict(beta=None)), (NULL, dict(out=None)), (ALIGN, dict(y=odd(1))), (ALIGN, dict(out=odd(4))),
                    (ALIGN, dict(beta=odd(3)))]:
        assert fwd(**e) == want, ("fwd", e)
    need = lib.mtlora_sum_ln_add_bwd_scratch_bytes(3, 12, 64, L.F32)
    assert need > 256
    for want, e in [(NULL, dict(dout=None)), (NULL, dict(dy_t=None)), (NULL, dict(dy_t=arr(9, null=1))), (NULL, dict(scratch=None)),
                    (NULL, dict(dgamma=None)), (NULL, dict(dbeta=None)), (ALIGN, dict(dout=odd(7))), (ALIGN, dict(dy_t=arr(9, odd=2))),
                    (ALIGN, dict(add=arr(8, odd=0))), (ALIGN, dict(scratch=odd(12))), (WORK, dict(scratch_bytes=need - 256 - 1)),
                    (WORK, dict(scratch_bytes=0)), (WORK, dict(scratch_bytes=-1))]:
        assert bwd(**e) == want, ("bwd", e)
    # no rows: OK without a launch, whatever the pointers (tensors without rows have no address); the limits still hold
    assert fwd(M=0) == OK and fwd(M=0, y=None, out=None, y_t=arr(0, null=1)) == OK and fwd(M=0, N=4096, dtype=L.BF16) == OK
    assert fwd(M=0, n=9) == SHAPE and fwd(M=0, N=100, dtype=L.BF16) == SHAPE
    assert bwd(M=0, dgamma=None, dbeta=None, dout=None) == OK  # (with dgamma / dbeta the empty backward zero-fills them on the device)
    # the size query answers -1 outside the limits
    q = lib.mtlora_sum_ln_add_bwd_scratch_bytes
    assert q(0, 12, 64, L.F32) == -1 and q(9, 12, 64, L.F32) == -1 and q(2, 12, 100, L.BF16) == -1 and q(2, 12, 4100, L.F32) == -1
    assert q(2, 12, 64, 7) == -1 and q(2, -1, 64, L.F32) == -1 and q(8, 0, 4096, L.F32) > 0 and q(1, 5, 4096, L.BF16) > 0


def test_addition_layer_on_cpu_keeps_the_aten_form(golden, monkeypatch):
    """off the device the layer's tail is the ATen expression it always was (the fused call needs device tensors): the linear call
    underneath is replaced by the oracle's parts, the tail is compared bit for bit"""
    from mtlora_amd import functional as Fn
    from mtlora_amd.lora import MTLoRALinear
    c = _case(golden)
    tasks = c["tasks"]
    K, N = c["params"]["linear.weight"].shape[1], c["params"]["linear.weight"].shape[0]
    m = MTLoRALinear(K, N, r=c["r"], lora_shared_scale=c["scale_s"], lora_task_scale=c["scale_t"], lora_dropout=0.0, tasks=tasks,
                     shared_mode="addition", bias=True)
    m.load_state_dict({k: v.float() for k, v in c["params"].items()})
    y0 = _pretrained(c).float()
    ys = [c["y_tasks"][t].float() for t in tasks]

    class FakeLinearFn:
        @staticmethod
        def apply(*args):
            return (y0,) + tuple(ys)

    monkeypatch.setattr(Fn, "MTLoRALinearFn", FakeLinearFn)
    assert not Fn.sum_norm_add_ok(m.lora_norm, y0, ys)
    y, yt = m(c["x"].float(), {t: c["x_tasks"][t].float() for t in tasks})
    tot = torch.stack(ys, 0).sum(0).float()
    want = y0 + torch.nn.functional.layer_norm(tot, (N,), m.lora_norm.weight.float(), m.lora_norm.bias.float(), m.lora_norm.eps).to(y0.dtype)
    assert torch.equal(y, want)
    assert all(yt[t] is ys[i] for i, t in enumerate(tasks))
    assert [n for n, _ in m.named_parameters() if "lora_norm" in n] == ["lora_norm.weight", "lora_norm.bias"]
