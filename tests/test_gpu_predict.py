"""GPU tests of the prediction path: csrc/predict.hip (through functional.upsample_predict), evaluation.get_output_low and
mtl_harness.predict_step / predict.

The expected values are an fp64 restatement written HERE, by the method of tests/test_gpu_eval.py: the same (dtype-rounded)
low-resolution tensor, upcast, F.interpolate in fp64 on the CPU, then get_output's formulas.  Only the kernel's fp32 arithmetic
differs.  The low-resolution inputs are those of test_gpu_eval.py (its make_case draws ``low`` first, so the same generator
and seed give the same tensor; its quantise recipe is restated below).

delta = 16 fp32 ulps of the largest |interpolated value| of the tensor (the margin test_gpu_eval.py derives for this
arithmetic); for the kinds whose values live in [0, 255] it is 16 ulps of 255 = 2.4e-4.

1. argmax     equal to the fp64 argmax at every pixel whose top-two margin is >= delta; the ambiguous share of the inputs is
              <= 1e-3 (asserted on the fp64 side, before the GPU is used); an exact tie resolves to the lower index.
2. fp32       max |kernel - fp64| <= delta (normals: the inputs have no pixel with |up| < 1e-4).
3. uint8      |kernel - floor(fp64)| <= 1 everywhere, equal wherever the fp64 value is further than delta from an integer;
              the share of such ambiguous values is <= 2e-3 (expected: 2 delta = 5e-4), asserted on the fp64 side.
4. every element written and nothing else (0xA5 / NaN prefill, 256-byte guards, bit-identical to the result without out=).
5. two launches give torch.equal results.
6. predict_step against validate_step through the torch meters, and its side effects (none).
7. predict_step against model(x, upsample=True) + get_output under the same autocast.

The model of items 6 and 7 is test_gpu_eval.py's small model (Swin-T at 224 px, ranks 16 / 4, heads at 28 x 28, predict
launches at scale 8): the window is 7, so a 64 px image (a 16 x 16 patch grid) cannot be built, and the heads' channel widths
are those of the four-stage model.

With MTLORA_PREDICT_FIGURES=<file> every measured figure is appended to that file (profiles/predict_gpu_tests.txt).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

AMBIGUOUS_SHARE = 1e-3
AMBIGUOUS_U8_SHARE = 2e-3
DELTA_255 = 16.0 * float(np.spacing(np.float32(255.0)))  # 2.4e-4
KIND_OF = {"semseg": "argmax", "human_parts": "argmax", "semseg40": "argmax", "normals": "normals", "sal": "sigmoid",
           "edge": "sigmoid", "depth": "identity"}
CH = {"semseg": 21, "human_parts": 7, "semseg40": 40, "normals": 3, "sal": 1, "depth": 1, "edge": 1}
GEOM = [(2, 56, 56, 8),   # the heads' geometry
        (2, 26, 30, 4),   # non-square, width not a multiple of the 16-column tile, a partial last row tile
        (4, 33, 70, 1),   # scale 1: W = 70, uint8 rows are not 4-byte aligned
        (1, 10, 21, 8),   # width not a multiple of the 8-column tile, a partial last row tile
        (2, 21, 27, 3)]   # W = 81, odd; 63 of the 64 lanes carry a column
DTYPES = [torch.float32, torch.bfloat16]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def figure(line):
    print(line)
    path = os.environ.get("MTLORA_PREDICT_FIGURES")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def make_low(task, B, h, w, S, seed):
    """the low-resolution tensor of test_gpu_eval.make_case(task, B, h, w, S, seed) (its first draw)"""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, h, w, CH[task], generator=g)
    if task == "depth":
        low = 3.0 + 0.8 * low
    elif task == "edge":
        low = low - 1.0
    return low


def quantise(low, dtype):
    """the low-resolution tensor in the kernel's input dtype.  bf16 keeps 8 bits, so two of C random logits of a pixel tie
    EXACTLY for about 1 pixel in 100; where the interpolation copies a source pixel (scale 1, clamped borders) that tie
    survives and is a margin of 0.  Such inputs do not meet the ambiguity condition whatever the seed, so the winner of a
    tied low-resolution pixel is moved up by two bf16 steps (test_gpu_eval.quantise)."""
    q = low.to(dtype)
    if dtype == torch.bfloat16 and low.shape[-1] > 4:
        f = q.float()
        top = f.topk(2, dim=-1)
        tie = top.values[..., 0] == top.values[..., 1]
        bumped = top.values[..., 0] + top.values[..., 0].abs().clamp_min(0.01) * 2.0 ** -6
        f.scatter_(-1, top.indices[..., :1], torch.where(tie, bumped, top.values[..., 0]).unsqueeze(-1))
        q = f.to(dtype)
    return q


def up64(low_q, S):
    """(B, H, W, C) fp64 bilinear upsample of the dtype-rounded low-resolution tensor"""
    return F.interpolate(low_q.double().permute(0, 3, 1, 2), scale_factor=S, mode="bilinear").permute(0, 2, 3, 1).contiguous()


def reference(kind, up):
    """fp64 get_output of the (B, H, W, C) upsampled tensor.  argmax: (class ids, ambiguous mask); else (values, delta)."""
    delta = 16.0 * float(np.spacing(np.float32(up.abs().max().item())))
    if kind == "argmax":
        top = up.topk(2, dim=-1)
        return top.indices[..., 0].to(torch.uint8), (top.values[..., 0] - top.values[..., 1]) < delta
    if kind == "normals":
        nrm = up.norm(dim=-1, keepdim=True)
        assert int((nrm < 1e-4).sum()) == 0, "input condition: no pixel with a vanishing normal"
        return (up / nrm.clamp_min(1e-12) + 1.0) * 255 / 2.0, DELTA_255
    if kind == "sigmoid":
        return (255 * 1 / (1 + torch.exp(-up)))[..., 0], DELTA_255
    return up, delta


@functools.lru_cache(maxsize=None)
def case(task, B, h, w, S, dtype):
    """(low in the kernel's dtype, fp64 reference) of one case: computed once, shared by the tests, never modified"""
    low_q = quantise(make_low(task, B, h, w, S, seed=7 * h + w + S), dtype)
    return low_q, reference(KIND_OF[task], up64(low_q, S))


def check_argmax(what, got, ref):
    am, amb = ref
    share = amb.float().mean().item()
    assert share <= AMBIGUOUS_SHARE, (what, share)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == am.shape, (got.dtype, got.shape)
    wrong = (got != am) & ~amb
    figure(f"{what}: ambiguous share {share:.3e}, differing pixels {int((got != am).sum())} (all ambiguous: {not bool(wrong.any())})")
    assert not bool(wrong.any()), (what, int(wrong.sum()))


def check_float(what, got, ref):
    val, delta = ref
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == val.shape, (got.dtype, got.shape, val.shape)
    err = (got.double() - val).abs().max().item()
    figure(f"{what}: max |kernel - fp64| {err:.3e} (delta {delta:.3e})")
    assert err <= delta, (what, err, delta)


def check_uint8(what, got, ref):
    val, delta = ref
    near = (val - val.round()).abs() <= delta  # within delta of an integer: the truncation may go either way
    share = near.float().mean().item()
    assert share <= AMBIGUOUS_U8_SHARE, (what, share)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == val.shape, (got.dtype, got.shape, val.shape)
    diff = (got.double() - val.floor()).abs()
    figure(f"{what}: ambiguous share {share:.3e}, max |kernel - floor(fp64)| {int(diff.max())}, differing {int((diff != 0).sum())}")
    assert diff.max().item() <= 1, (what, diff.max().item())
    assert not bool(((diff != 0) & ~near).any()), (what, int(((diff != 0) & ~near).sum()))


def name(task, B, h, w, S, dtype, extra=""):
    return f"{task}{extra} {B}x{h}x{w} S{S} {str(dtype).replace('torch.', '')}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,w,S", GEOM)
@pytest.mark.parametrize("task", ["semseg", "human_parts", "semseg40"])
def test_argmax_vs_fp64(task, B, h, w, S, dtype):
    from mtlora_amd import functional as Fn
    low_q, ref = case(task, B, h, w, S, dtype)
    assert ref[1].float().mean().item() <= AMBIGUOUS_SHARE  # the inputs' condition, before the GPU is used
    check_argmax(name(task, B, h, w, S, dtype), Fn.upsample_predict("argmax", low_q.to(dev()), S), ref)


@pytest.mark.parametrize("task", ["depth", "normals"])
def test_fp16_input_vs_fp64(task):
    """the fp16 branch of the host's dtype ladder (DTYPES above covers fp32 and bf16): the same bound on the fp16-rounded input"""
    from mtlora_amd import functional as Fn
    B, h, w, S = 1, 10, 21, 8
    low_q, ref = case(task, B, h, w, S, torch.float16)
    check_float(name(task, B, h, w, S, torch.float16), Fn.upsample_predict(KIND_OF[task], low_q.to(dev()), S), ref)


def test_argmax_exact_tie_takes_the_lower_index():
    """scale 1 copies the source pixel (both weights of the second corner are exactly 0), so equal bf16 logits stay equal:
    the class id must be torch.max's, the FIRST maximum."""
    from mtlora_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    low = torch.randn(1, 9, 70, 21, generator=g).to(torch.bfloat16)
    low[0, 0, 0, 5] = low[0, 0, 0, 12] = 6.0      # a corner
    low[0, 4, 33, 0] = low[0, 4, 33, 20] = 7.0    # first and last class
    low[0, 8, 69, 19] = low[0, 8, 69, 20] = 5.0   # the last pixel
    low[0, 2, 64:70, 3] = 4.5                     # a run in the second column tile, three-way
    low[0, 2, 64:70, 9] = 4.5
    low[0, 2, 64:70, 17] = 4.5
    want = torch.max(low.float(), dim=3)[1]
    assert (want[0, 0, 0], want[0, 4, 33], want[0, 8, 69], want[0, 2, 66]) == (5, 0, 19, 3)
    got = Fn.upsample_predict("argmax", low.to(dev()), 1).cpu()
    assert torch.equal(got.long(), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,w,S", GEOM)
@pytest.mark.parametrize("task", ["normals", "sal", "edge", "depth"])
def test_fp32_outputs_vs_fp64(task, B, h, w, S, dtype):
    from mtlora_amd import functional as Fn
    low_q, ref = case(task, B, h, w, S, dtype)
    check_float(name(task, B, h, w, S, dtype), Fn.upsample_predict(KIND_OF[task], low_q.to(dev()), S), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,w,S", GEOM)
@pytest.mark.parametrize("task", ["normals", "sal", "edge"])
def test_uint8_outputs_vs_fp64(task, B, h, w, S, dtype):
    from mtlora_amd import functional as Fn
    low_q, ref = case(task, B, h, w, S, dtype)
    near = (ref[0] - ref[0].round()).abs() <= ref[1]
    assert near.float().mean().item() <= AMBIGUOUS_U8_SHARE  # the inputs' condition, before the GPU is used
    got = Fn.upsample_predict(KIND_OF[task], low_q.to(dev()), S, out_dtype=torch.uint8)
    check_uint8(name(task, B, h, w, S, dtype, " uint8"), got, ref)


@pytest.mark.parametrize("task", ["semseg", "normals", "sal", "depth"])
def test_fp16_input_vs_fp64(task):
    """the third input dtype, on the geometry with partial tiles in both directions"""
    from mtlora_amd import functional as Fn
    B, h, w, S = 2, 26, 30, 4
    low_q = make_low(task, B, h, w, S, seed=7 * h + w + S).to(torch.float16)
    kind = KIND_OF[task]
    ref = reference(kind, up64(low_q, S))
    got = Fn.upsample_predict(kind, low_q.to(dev()), S)
    if kind == "argmax":
        check_argmax(name(task, B, h, w, S, torch.float16), got, ref)
    else:
        check_float(name(task, B, h, w, S, torch.float16), got, ref)


GUARD = 256


@pytest.mark.parametrize("B,h,w,S", [(4, 33, 70, 1), (2, 21, 27, 3)])
@pytest.mark.parametrize("task,out_dtype", [("semseg", torch.uint8), ("normals", torch.float32), ("normals", torch.uint8),
                                            ("sal", torch.float32), ("sal", torch.uint8), ("depth", torch.float32)])
def test_every_element_written_and_nothing_else(task, out_dtype, B, h, w, S):
    from mtlora_amd import functional as Fn
    kind = KIND_OF[task]
    low = case(task, B, h, w, S, torch.float32)[0].to(dev())
    plain = Fn.upsample_predict(kind, low, S, out_dtype=out_dtype)
    n = plain.numel()
    if out_dtype == torch.uint8:
        buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev())
        lo, hi = GUARD, GUARD + n
    else:
        buf = torch.full((n + 2 * GUARD // 4,), float("nan"), dtype=torch.float32, device=dev())
        lo, hi = GUARD // 4, GUARD // 4 + n
    pattern = buf[:lo].clone()
    out = buf[lo:hi].view(plain.shape)
    got = Fn.upsample_predict(kind, low, S, out=out)
    assert got.data_ptr() == out.data_ptr()
    head, tail = buf[:lo].view(torch.uint8), buf[hi:].view(torch.uint8)
    assert torch.equal(head, pattern.view(torch.uint8)) and torch.equal(tail, pattern.view(torch.uint8)), "guard bytes were written"
    if out_dtype == torch.float32:
        assert not bool(torch.isnan(out).any()), "an element was not written"
    assert torch.equal(out.view(torch.uint8), plain.view(torch.uint8))
    with pytest.raises(RuntimeError, match="out must be"):
        Fn.upsample_predict(kind, low, S, out=out.flatten())
    with pytest.raises(RuntimeError):
        Fn.upsample_predict(kind, low, S, out=out.to(torch.float64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_launches_give_equal_results(dtype):
    from mtlora_amd import functional as Fn
    B, h, w, S = GEOM[0]
    for task, ods in (("semseg", (torch.uint8,)), ("normals", (torch.float32, torch.uint8)), ("sal", (torch.float32, torch.uint8)),
                      ("depth", (torch.float32,))):
        low = case(task, B, h, w, S, dtype)[0].to(dev())
        for od in ods:
            a = Fn.upsample_predict(KIND_OF[task], low, S, out_dtype=od)
            b = Fn.upsample_predict(KIND_OF[task], low, S, out_dtype=od)
            assert torch.equal(a, b), (task, od)


def test_get_output_low_shapes_and_dtypes():
    """get_output's shapes for B > 1 (the batch axis of one image is kept); uint8 class maps; uint8=True for the images"""
    from mtlora_amd.evaluation import get_output, get_output_low
    for task, C in (("semseg", 21), ("human_parts", 7), ("normals", 3), ("sal", 1), ("edge", 1), ("depth", 1)):
        for B in (2, 1):
            low = torch.randn(B, 5, 6, C, device=dev())
            a = get_output_low(low, task, 4)
            u = get_output_low(low, task, 4, uint8=True)
            want = get_output(F.interpolate(low.permute(0, 3, 1, 2), scale_factor=4, mode="bilinear"), task)
            if B > 1:
                assert a.shape == want.shape, (task, a.shape, want.shape)
            assert a.shape[0] == B and a.shape[1:3] == (20, 24) and u.shape == a.shape
            assert a.dtype == (torch.uint8 if task in ("semseg", "human_parts") else torch.float32)
            assert u.dtype == (torch.float32 if task == "depth" else torch.uint8)


# ------------------------------------------------------------------------------------------------
# predict_step / predict on a small model
# ------------------------------------------------------------------------------------------------
TASKS = ("semseg", "normals", "sal", "depth")
IMG = 224


@pytest.fixture(scope="module")
def small():
    """Swin-T at 224 px (heads at 28 x 28, scale 8), BatchNorm statistics warmed, depth predictions away from 0"""
    from mtlora_amd import mtl_harness as H
    model = H.build_model(img_size=IMG, tasks=TASKS, r_shared=16, r_task=4, seed=0).to(dev())
    model.train()
    with torch.no_grad():
        for s in range(2):
            img, _ = H.synthetic_batch(2, IMG, TASKS, seed=50 + s, device=dev())
            model(img, upsample=False)
        model.decoders.decoders["depth"].last_layer[3].bias.fill_(3.0)
    return model


def _state(meter, task):
    m = meter.meters[task]
    c = m.counts.cpu().numpy()
    per = torch.cat(m.per_image).cpu().numpy().reshape(-1) if task == "sal" else np.zeros(0, np.int64)
    return c, per, (m.sums.cpu().tolist() if task in ("normals", "depth") else [])


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_predict_step_agrees_with_validate_step(small, amp):
    """PerformanceMeter.update on predict_step's fp32 predictions against the meter state validate_step leaves for the same
    batch: counts within 1e-3 of the pixels they are taken over (both routes decide from values that may differ by delta: the
    ambiguity cap of item 1), float sums to 1e-4 relative (two fp32 routes; one route against fp64 is held to 1e-5).  No side
    effects: training flag, parameters and buffers (num_batches_tracked included) bit-identical."""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter
    model = small.train()
    crit = H.MultiTaskLoss(TASKS)
    img, tg = H.synthetic_batch(2, IMG, TASKS, seed=11, device=dev())
    tg["sal"][-1] = 0.0
    fused, plain = PerformanceMeter(TASKS), PerformanceMeter(TASKS)
    H.validate_step(model, crit, fused, img, tg, amp_dtype=amp)
    before = {k: v.detach().clone() for k, v in list(model.named_parameters()) + list(model.named_buffers())}
    assert any(k.endswith("num_batches_tracked") for k in before)
    pred = H.predict_step(model, img, amp_dtype=amp)
    assert model.training and set(pred) == set(TASKS)
    after = dict(list(model.named_parameters()) + list(model.named_buffers()))
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert pred["semseg"].dtype == torch.uint8 and pred["semseg"].shape == (2, IMG, IMG)
    assert pred["normals"].shape == (2, IMG, IMG, 3) and pred["sal"].shape == (2, IMG, IMG) and pred["depth"].shape == (2, IMG, IMG, 1)
    plain.update(pred, tg)
    npix = 2 * IMG * IMG
    for t in TASKS:
        (c1, p1, s1), (c2, p2, s2) = _state(fused, t), _state(plain, t)
        dc = int(np.abs(c1 - c2).max())
        dp = int(np.abs(p1 - p2).max()) if len(p1) else 0
        ds = max([abs(a - b) / max(abs(b), 1e-300) for a, b in zip(s1, s2)], default=0.0)
        figure(f"predict_step vs validate_step {t} amp={amp}: max count diff {dc} (cap {int(1e-3 * npix)}), per-image {dp} "
               f"(cap {int(1e-3 * npix / 2)}), float sums rel {ds:.3e}")
        assert dc <= 1e-3 * npix and dp <= 1e-3 * npix / 2 and ds <= 1e-4, (t, dc, dp, ds)
    # predict(): a generator over batches, tuples as a loader yields them included; a subset of the tasks
    outs = list(H.predict(model, [(img, tg), img], tasks=("sal", "semseg"), amp_dtype=amp))
    assert len(outs) == 2 and all(set(o) == {"sal", "semseg"} for o in outs)
    for o in outs:
        assert torch.equal(o["sal"], pred["sal"]) and torch.equal(o["semseg"], pred["semseg"])
    u8 = H.predict_step(model, img, uint8=True, amp_dtype=amp)
    assert u8["sal"].dtype == u8["normals"].dtype == u8["semseg"].dtype == torch.uint8 and u8["depth"].dtype == torch.float32
    assert torch.equal(u8["sal"], pred["sal"].to(torch.uint8)) and torch.equal(u8["normals"], pred["normals"].to(torch.uint8))
    assert torch.equal(u8["semseg"], pred["semseg"]) and torch.equal(u8["depth"], pred["depth"])


def _check_against_own_low(model, img, pred, what):
    """predict_step's outputs against the fp64 restatement on the model's own low-resolution outputs (items 1 and 2)"""
    model.eval()
    with torch.no_grad():
        low = model(img, upsample=False)
    for t in TASKS:
        ref = reference(KIND_OF[t], up64(low[t].float().cpu(), IMG // low[t].shape[1]))
        if KIND_OF[t] == "argmax":
            check_argmax(f"{what} {t}", pred[t], ref)
        else:
            check_float(f"{what} {t}", pred[t], ref)


def test_predict_step_on_a_merged_model(small):
    """merged and unmerged: each state's predictions are held to the fp64 restatement on that state's own low-resolution
    outputs by items 1 and 2, the merged state survives predict_step, and the two states' predictions differ by no more than
    the merge itself moves the outputs (W + s B A is rounded once in fp32: 1e-3 of the range, the bound of the merge tests)."""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.checkpoint import merge_lora_weights, unmerge_lora_weights
    from mtlora_amd.lora import MTLoRALinear
    model = small.eval()
    img, _ = H.synthetic_batch(2, IMG, TASKS, seed=12, device=dev())
    un = H.predict_step(model, img, amp_dtype=None)
    _check_against_own_low(model, img, un, "unmerged")
    assert merge_lora_weights(model.backbone) > 0
    try:
        merged_flags = [m.merged for m in model.modules() if isinstance(m, MTLoRALinear)]
        me = H.predict_step(model, img, amp_dtype=None)
        assert [m.merged for m in model.modules() if isinstance(m, MTLoRALinear)] == merged_flags and any(merged_flags)
        _check_against_own_low(model, img, me, "merged")
    finally:
        unmerge_lora_weights(model.backbone)
    same = (un["semseg"] == me["semseg"]).float().mean().item()
    figure(f"merged vs unmerged: class maps agree on {same:.5f}")
    assert same >= 0.99
    for t in ("normals", "sal", "depth"):
        d = (un[t] - me[t]).abs().max().item()
        rng = 255.0 if t != "depth" else un[t].abs().max().item()
        figure(f"merged vs unmerged {t}: max |difference| {d:.3e} (range {rng:.3g})")
        assert d <= 1e-3 * rng, (t, d)
    model.train()


def test_predict_step_vs_the_full_resolution_route(small):
    """model(x, upsample=True) + get_output under the same bf16 autocast.  That route rounds the upsampled logits to bf16, so
    near-ties go either way: class maps agree on >= 99 % of the pixels, float maps within 1.0 on the 0..255 scale (more than the
    bf16 rounding of a value up to 255 moves it, less than any real bug); the depth within 2^-8 of its largest value (a bf16
    rounding is at most 2^-9 relative)."""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import get_output
    model = small.eval()
    img, _ = H.synthetic_batch(2, IMG, TASKS, seed=13, device=dev())
    pred = H.predict_step(model, img)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        full = model(img, upsample=True)
    old = {t: get_output(full[t].float(), t) for t in TASKS}
    share = (pred["semseg"].long() == old["semseg"]).float().mean().item()
    figure(f"predict_step vs full-resolution route: class maps agree on {share:.5f}")
    assert share >= 0.99
    for t in ("normals", "sal"):
        d = (pred[t] - old[t]).abs().max().item()
        figure(f"predict_step vs full-resolution route {t}: max |difference| {d:.3e} on 0..255")
        assert d <= 1.0, (t, d)
    d, top = (pred["depth"] - old["depth"]).abs().max().item(), old["depth"].abs().max().item()
    figure(f"predict_step vs full-resolution route depth: max |difference| {d:.3e} (largest value {top:.3g})")
    assert d <= top * 2.0 ** -8
    model.train()
