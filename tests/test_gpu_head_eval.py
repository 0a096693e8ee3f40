"""The decoder head in eval mode as one launch (csrc/head_eval.hip, Fn.head_eval): the kernel against the portable definition in fp64
on the 16-bit-rounded operands, relu=False / non-finite containment / class padding, the HighResolutionHead route and its operand
cache, and graph capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.bfloat16: 1e-2, torch.float16: 2e-3}  # the project's 16-bit tolerances, relative to max |ref|


def _operands(M, ldx, Hd, classes, dtype, seed=0):
    """x, w1p, a, c, w2p, b2 as the kernel takes them: a, c from non-trivial BatchNorm statistics, class padding zero"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    ncp = classes + (-classes) % 8
    mean, var, gamma, beta, b1 = 0.3 * r(Hd), 0.5 + torch.rand(Hd, generator=g), 1.0 + 0.2 * r(Hd), 0.3 * r(Hd), 0.2 * r(Hd)
    a = gamma / torch.sqrt(var + 1e-5)
    c = beta + (b1 - mean) * a
    w2p, b2 = torch.zeros(ncp, Hd), torch.zeros(ncp)
    w2p[:classes], b2[:classes] = r(classes, Hd) / Hd ** 0.5, 0.2 * r(classes)
    ops = (r(M, ldx).to(dtype), (r(Hd, ldx) / ldx ** 0.5).to(dtype), a, c, w2p.to(dtype), b2)
    return tuple(t.to(DEV).contiguous() for t in ops)


def _ref(ops, relu=True):
    from mtlora_amd import functional as Fn
    return Fn.head_eval_torch(*[t.double() for t in ops], relu=relu)


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,ldx,Hd,classes", [(1, 16, 8, 1), (33, 48, 40, 3), (130, 272, 1080, 21), (257, 272, 1080, 40),
                                              (4 * 128 + 5, 272, 96, 7), (70, 512, 72, 9)])
def test_kernel_against_fp64(M, ldx, Hd, classes, dtype):
    """a single row, ragged waves and row blocks, the hidden tail (8, 40, 1080) and a whole number of chunks (96), one and two class
    tiles, class padding; (70, 512, 72, 9) is the widest input the kernel takes (its own instantiation).  1x the 16-bit tolerance:
    the intermediate is rounded once to 16 bits (2^-9 / 2^-11 per element, averaged over Hd terms), the output once"""
    from mtlora_amd import functional as Fn
    ops = _operands(M, ldx, Hd, classes, dtype)
    got = Fn.head_eval(*ops, relu=True)
    assert got.shape == (M, ops[4].shape[0]) and got.dtype == dtype
    err = _rel(got, _ref(ops))
    print(f"head_eval M={M} ldx={ldx} Hd={Hd} classes={classes} {dtype}: rel err {err:.3e} (tol {TOL[dtype]:.0e})")
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_identity_nonfinite_row_and_class_padding(dtype):
    from mtlora_amd import functional as Fn
    ops = _operands(33, 48, 40, 3, dtype, seed=1)
    clean = Fn.head_eval(*ops, relu=False)
    err = _rel(clean, _ref(ops, relu=False))
    print(f"head_eval relu=False {dtype}: rel err {err:.3e}")
    assert err <= TOL[dtype], err
    assert _rel(clean, _ref(ops, relu=True)) > 10 * TOL[dtype]  # (the clamp matters on these operands)
    assert bool((clean[:, 3:] == 0).all())  # zero weight rows + zero bias
    x = ops[0].clone()
    x[7, 5] = float("nan")
    for relu in (True, False):
        base, bad = Fn.head_eval(*ops, relu=relu), Fn.head_eval(x, *ops[1:], relu=relu)
        assert not bool(torch.isfinite(bad[7, :3]).any())
        keep = torch.arange(33, device=DEV) != 7
        assert torch.equal(bad[keep], base[keep])


def _head_and_maps():
    from mtlora_amd import mtl_harness as H
    torch.manual_seed(0)
    head = H.HighResolutionHead((18, 36, 72, 144), 21).to(DEV)
    bn = head.last_layer[1]
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.normal_(1.0, 0.2)
        bn.bias.normal_(0, 0.3)
    maps = [torch.randn(1, 16 >> i, 16 >> i, c, device=DEV).bfloat16().permute(0, 3, 1, 2) for i, c in enumerate((18, 36, 72, 144))]
    return H, head.eval(), maps


def test_module_route(monkeypatch):
    from mtlora_amd import functional as Fn
    H, head, maps = _head_and_maps()
    tol = TOL[torch.bfloat16]

    def run(on):
        monkeypatch.setattr(H, "HEAD_EVAL", on)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return head(maps, channels_last_out=True).reshape(256, 21)

    def ref():
        t = Fn.ConcatUpsampleFn.apply(*[m.permute(0, 2, 3, 1) for m in maps])
        return Fn.head_eval_torch(t.double(), *[o.double() for o in head._head_eval_operands(t, head._col_idx)])[:, :21]

    on, off = run(True), run(False)
    assert on.dtype == off.dtype == torch.bfloat16 and "_he_cache" in head.__dict__
    e_ref, e_off = _rel(on, ref()), _rel(on, off.double())
    print(f"head route: fused vs fp64 {e_ref:.3e}, fused vs four steps {e_off:.3e}")
    assert e_ref <= tol and e_off <= 2 * tol
    head.last_layer[1].running_var.mul_(4.0)  # in place: the cached operands follow ``_version``
    moved = run(True)
    assert not torch.equal(moved, on) and _rel(moved, ref()) <= tol
    head.train()  # the new route must not engage
    assert torch.equal(run(True), run(False))


def test_capture_replays_bit_equal():
    from mtlora_amd import functional as Fn
    ops = _operands(130, 272, 1080, 21, torch.bfloat16, seed=2)
    eager = Fn.head_eval(*ops)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = Fn.head_eval(*ops)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
