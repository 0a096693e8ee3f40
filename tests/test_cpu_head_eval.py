"""The eval-mode decoder head without a GPU: the portable definition ``functional.head_eval_torch`` against the literal layer sequence
in fp64, and the return code of ``mtlora_head_eval_fwd`` for calls with one defect each, all rejected on the host."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("relu", [True, False])
def test_head_eval_torch_is_the_layer_sequence(relu):
    from mtlora_amd import functional as Fn
    torch.manual_seed(0)
    K, Hd, nc = 12, 24, 5
    c0, bn, c3 = torch.nn.Conv2d(K, Hd, 1).double(), torch.nn.BatchNorm2d(Hd).double().eval(), torch.nn.Conv2d(Hd, nc, 1).double()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(1.0, 0.3)
        bn.bias.normal_(0, 0.5)
        x = torch.randn(2, K, 3, 4, dtype=torch.float64)
        h = F.batch_norm(c0(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, bn.momentum, bn.eps)
        want = c3(F.relu(h) if relu else h).permute(0, 2, 3, 1).reshape(-1, nc)
        a, c = Fn.head_eval_affine(bn, c0.bias)
        got = Fn.head_eval_torch(x.permute(0, 2, 3, 1).reshape(-1, K), c0.weight.view(Hd, K), a.double(), c.double(), c3.weight.view(nc, Hd),
                                 c3.bias, relu=relu)
    assert a.dtype == torch.float32  # (the kernel's operand type: the comparison carries its rounding)
    assert ((got - want).abs().max() / want.abs().max()).item() <= 1e-6


def test_host_rejects_every_single_defect():
    from mtlora_amd import _lib as L
    lib = L.lib()
    OK, DTYPE, SHAPE, ALIGN, NULL, UNSUP = 0, -1, -2, -3, -4, -7
    names = ("X", "W1", "a", "c", "W2", "b2", "O")
    good = dict({n: 4096 * (j + 1) for j, n in enumerate(names)}, M=100, ldx=272, Hd=1080, ncp=24, dtype=L.BF16)  # (fake addresses)

    def call(**e):
        q = {**good, **e}
        return lib.mtlora_head_eval_fwd(*[ctypes.c_void_p(q[n]) for n in names], q["M"], q["ldx"], q["Hd"], q["ncp"], 1, q["dtype"], None)

    cases = [(DTYPE, dict(dtype=7)), (UNSUP, dict(dtype=L.F32)), (SHAPE, dict(ldx=12)), (SHAPE, dict(ncp=21)), (SHAPE, dict(M=-1)),
             (SHAPE, dict(Hd=0)), (UNSUP, dict(Hd=1084)), (UNSUP, dict(ncp=72)), (UNSUP, dict(ldx=520))]
    cases += [(NULL, {n: None}) for n in names] + [(ALIGN, {n: good[n] + 8}) for n in names]
    for want, e in cases:
        assert call(**e) == want, e
    # no rows: OK before a pointer or a shape is looked at; the order is dtype, M == 0, null, alignment, shape
    assert call(M=0, X=None, ldx=12) == OK and call(M=0, dtype=L.F32) == UNSUP
    assert call(X=None, O=good["O"] + 8, ldx=12) == NULL and call(O=good["O"] + 8, ldx=12) == ALIGN
    q = lib.mtlora_head_eval_supported
    assert q(401408, 272, 1080, 24, L.BF16) == 1 and q(1, 8, 8, 8, L.F16) == 1 and q(0, 512, 8, 64, L.BF16) == 1
    assert q(100, 272, 1080, 24, L.F32) == 0 and q(100, 12, 1080, 24, L.BF16) == 0 and q(100, 272, 1084, 24, L.BF16) == 0
    assert q(100, 272, 1080, 72, L.BF16) == 0
