"""Decoder front end on the HIP path (csrc/decoder_front.hip): the stages' 1x1 convs, bilinear upsample and concat in one launch,
held to ``functional.decoder_front_torch`` in fp64 on the same 16-bit operands.  Bounds (u = 2^-8 bf16, 2^-10 fp16: one output
rounding with a 2x margin; A / S: the same evaluation on absolute values, which covers the fp32 accumulation over K <= 768):
forward and dx  |err| <= u |ref| + 1e-4 A,  dW  |err| <= u S."""
import pytest
import torch

from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
# (B, finest grid, scales, C, c, band_rows): (a) two images, H != W, pad columns 18-19, c no multiple of 16, ragged last band of
# the backward (8 + 4 rows); a5: the forward's ragged band too (5 + 5 + 2) | (b) two stages | (c) the real stage geometry
CASES = {"a": (2, (12, 8), (1, 2, 4, 4), (32, 64, 96, 96), (18, 36, 72, 144), 0),
         "a5": (2, (12, 8), (1, 2, 4, 4), (32, 64, 96, 96), (18, 36, 72, 144), 5),
         "b": (1, (8, 8), (1, 2), (32, 64), (6, 8), 0),
         "c": (1, (56, 56), (1, 2, 4, 4), (192, 384, 768, 768), (18, 36, 72, 144), 0)}
_REF = {}


def _case(name, dtype):
    """inputs (16-bit values) and the fp64 reference, computed once per (case, dtype)"""
    if (name, dtype) in _REF:
        return _REF[name, dtype]
    from mtlora_amd import functional as Fn
    B, (H, W), scales, Cs, cs, band = CASES[name]
    grids = [(H // s, W // s) for s in scales]
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(B, h * w, C, generator=g).to(dtype) for (h, w), C in zip(grids, Cs)]
    ws = [(0.2 * torch.randn(c, C, generator=g)).to(dtype) for c, C in zip(cs, Cs)]
    offs, ld = Fn.ConcatUpsampleFn.layout(cs)
    live = torch.zeros(ld, dtype=torch.bool)
    for o, c in zip(offs, cs):
        live[o:o + c] = True
    dout = torch.randn(B * H * W, ld, generator=g).to(dtype)
    dref = dout.double() * live
    x64, w64 = [x.double().requires_grad_(True) for x in xs], [w.double().requires_grad_(True) for w in ws]
    out = Fn.decoder_front_torch(x64, w64, grids)
    grads = torch.autograd.grad(out, x64 + w64, dref)
    xa, wa = [x.double().abs().requires_grad_(True) for x in xs], [w.double().abs().requires_grad_(True) for w in ws]
    A = Fn.decoder_front_torch(xa, wa, grids)
    A_dx = torch.autograd.grad(A, xa, dref.abs())
    S = []  # sum over pixels of |gz| |x|: gz from the same definition with identity weights
    for i, c in enumerate(cs):
        z = [torch.zeros(B, h * w, k, dtype=torch.float64, requires_grad=True) for (h, w), k in zip(grids, cs)]
        gz = torch.autograd.grad(Fn.decoder_front_torch(z, [torch.eye(k, dtype=torch.float64) for k in cs], grids), z[i], dref)[0]
        S.append(torch.einsum("blc,blk->ck", gz.abs(), xs[i].double().abs()))
    _REF[name, dtype] = dict(grids=grids, xs=xs, ws=ws, dout=dout, live=live, out=out.detach(), A=A.detach(), grads=grads, A_dx=A_dx, S=S,
                             band=band, n=len(cs))
    return _REF[name, dtype]


def _run(r, dtype):
    from mtlora_amd import functional as Fn
    xs = [x.to(dev()).requires_grad_(True) for x in r["xs"]]
    ws = [w.float().to(dev()).requires_grad_(True) for w in r["ws"]]
    out = Fn.DecoderFrontFn.apply(tuple(r["grids"]), dtype, r["band"], *xs, *ws)
    dout = r["dout"].clone()
    dout[:, ~r["live"]] = float("nan")  # the kernel must ignore the pad columns of the incoming gradient
    return out, xs + ws, dout.to(dev())


@pytest.mark.parametrize("dtype", list(U), ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_fp64(name, dtype):
    r, u = _case(name, dtype), U[dtype]
    out, leaves, dout = _run(r, dtype)
    grads = torch.autograd.grad(out, leaves, dout, retain_graph=True)
    again = torch.autograd.grad(out, leaves, dout)
    got = out.detach().cpu()
    assert got.dtype == dtype and got.shape == r["out"].shape
    assert (got[:, ~r["live"]].view(torch.int16) == 0).all(), "pad columns are not +0"
    err, bound = (got.double() - r["out"]).abs(), u * r["out"].abs() + 1e-4 * r["A"]
    print(f"decoder_front {name} {dtype}: forward max err / bound {(err / bound.clamp_min(1e-30))[:, r['live']].max().item():.3f}")
    assert (err <= bound).all()
    n = r["n"]
    for i in range(2 * n):
        a, b, ref = grads[i], again[i], r["grads"][i]
        assert torch.equal(a, b), f"backward output {i} differs between two calls"
        err = (a.detach().cpu().double().view(ref.shape) - ref).abs()
        bound = u * ref.abs() + 1e-4 * r["A_dx"][i] if i < n else u * r["S"][i - n]
        print(f"decoder_front {name} {dtype}: {'dx' if i < n else 'dW'}_{i % n} max err / bound {(err / bound.clamp_min(1e-30)).max().item():.3f}")
        assert (err <= bound).all(), i


def _downsampler(dims, chans, res):
    from mtlora_amd import mtl_harness as H
    torch.manual_seed(0)
    return H.Downsampler(dims, chans, res).to(dev())


@pytest.mark.parametrize("dims, fused", [((32, 64), True), ((24, 64), False)], ids=["supported", "C24"])
def test_module_routes_by_support(monkeypatch, dims, fused):
    """with the switch on a Downsampler hands over the fused pixel matrix where ``decoder_front_ok`` holds and keeps the separate
    steps for a shape ``mtlora_decoder_front_supported`` refuses (C_0 = 24); without autocast (fp32) it keeps them too"""
    from mtlora_amd import mtl_harness as H
    monkeypatch.setattr(H, "DECODER_FRONT", True)
    ds = _downsampler(dims, (8, 8), (8, 4))
    feats = [torch.randn(1, r * r, d, device=dev()) for r, d in zip((8, 4), dims)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert isinstance(ds(feats), H.DecoderFront) == fused
    assert isinstance(ds(feats), list)


def test_model_level_error_against_fp64(monkeypatch):
    """a small MultiTaskSwin, bf16 autocast, train mode, forward + backward with the switch on and off: per-task low-resolution
    outputs and the downsampler.*.weight gradients against the decoders run in fp64 on the CPU from the same stage tokens; the
    fused path's maximum error is at most twice the separate steps'"""
    import copy
    from mtlora_amd import mtl_harness as H
    tasks = ["semseg", "normals"]
    model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=3).to(dev()).train()
    img, _ = H.synthetic_batch(2, 224, tasks, seed=5, device=dev())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        stages = [{t: tl[t].detach() for t in tasks} for _, tl in model.backbone(img, return_stages=True)]
    g = torch.Generator().manual_seed(1)
    res = model.input_res[0]
    cot = {t: torch.randn(2, res, res, H.num_output(t), generator=g) for t in tasks}
    params = [f"{t}.downsample_{i}.weight" for t in tasks for i in range(4)]

    def run(down, dec, cast, device, amp):
        outs = {}
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            for t in tasks:
                outs[t] = dec({t: down[t]([cast(s[t]) for s in stages])}, upsample=False, tasks=[t])[t]
        named = dict(down.named_parameters())
        grads = torch.autograd.grad(sum((outs[t].double() * cot[t].to(device).double()).sum() for t in tasks), [named[n] for n in params])
        return [outs[t].detach().double().cpu() for t in tasks] + [q.double().cpu() for q in grads]

    ref = run(copy.deepcopy(model.downsampler).double().cpu(), copy.deepcopy(model.decoders).double().cpu().train(),
              lambda s: s.double().cpu(), torch.device("cpu"), False)
    errs = {}
    for on in (False, True):
        monkeypatch.setattr(H, "DECODER_FRONT", on)
        got = run(model.downsampler, copy.deepcopy(model.decoders).train(), lambda s: s, dev(), True)
        errs[on] = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(got, ref)]
    out_n = len(tasks)
    off_o, off_g, on_o, on_g = max(errs[False][:out_n]), max(errs[False][out_n:]), max(errs[True][:out_n]), max(errs[True][out_n:])
    print(f"decoder_front model level: outputs off {off_o:.3e} on {on_o:.3e}; downsampler weight gradients off {off_g:.3e} on {on_g:.3e}")
    assert on_o <= 2 * off_o and on_g <= 2 * off_g
