"""Partially labelled batches on the GPU (run on an MI355X: -m gpu): mtlora_upsample_loss_valid / mtlora_label_stat_valid
(csrc/loss.hip, csrc/reduce.hip) against the unchanged entries (bit for bit where every sample is labelled) and against
functional.upsample_loss_valid_torch in fp64; the unlabelled samples' prediction and label are never read (NaN / Inf / 0xFF
bytes in them change no bit); train_step(valid=) and GraphedTrainStep(valid=) on the small 2-stage model; the ingest of a
merged PASCAL + NYUD wire batch.

Shapes: B = 3, (h, w) = (5, 9) -- off the tile grid in both directions (TQ = 7, TR = 4 at scale 8) --, scale 8 (the compile-time
instantiation) and 4 (the run-time one).  Tolerances against fp64 are those of tests/test_gpu_kernels.py::
test_upsample_loss_vs_oracle: value 2e-5 (fp32) / 1e-2 (bf16) of max(1, |ref|), gradient 1e-4 / 1e-2 of its largest element.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, h, w = 3, 5, 9
MASKS = {"all": [1, 1, 1], "mid": [1, 0, 1], "last": [0, 0, 1], "none": [0, 0, 0]}
# name: (kind, C, pos_weight)
CASES = {"softmax21": ("softmax", 21, None), "normals3": ("normals", 3, None), "bce_stat": ("balanced_bce", 1, None),
         "bce_const": ("balanced_bce", 1, 0.95), "l1": ("l1_masked", 1, None)}


ERR_DTYPE, ERR_SHAPE, ERR_ALIGN, ERR_NULL, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -7  # include/mtlora_hip.h


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def make_case(kind, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(B, h, w, C, generator=g) * 2.0
    H, W = h * S, w * S
    if kind == "softmax":
        lab = torch.randint(0, C, (B, 1, H, W), generator=g).float()
        lab[torch.rand(B, 1, H, W, generator=g) < 0.07] = 255.0
    elif kind == "normals":
        lab = torch.nn.functional.normalize(torch.randn(B, 3, H, W, generator=g), dim=1)
        lab[torch.rand(B, 3, H, W, generator=g) < 0.05] = 255.0
    elif kind == "balanced_bce":  # a different share of positives per sample: w depends on which samples are labelled
        lab = (torch.rand(B, 1, H, W, generator=g) < torch.tensor([0.15, 0.3, 0.6]).view(B, 1, 1, 1)).float()
    else:
        lab = torch.rand(B, 1, H, W, generator=g) * 10
        lab[torch.rand(B, 1, H, W, generator=g) < 0.07] = 255.0
    return low, lab


def run(kind, low, lab, S, pw, valid):
    """(loss, d loss / d low) of one call on the GPU; the gradient is the kernel's dlow (times 1.0)"""
    from mtlora_amd import functional as Fn
    x = low.clone().requires_grad_(True)
    if valid is None:
        got = Fn.UpsampleLossFn.apply(kind, x, lab, S, 255.0, pw)
    else:
        got = Fn.UpsampleLossFn.apply(kind, x, lab, S, 255.0, pw, valid)
    got.backward()
    return got.detach(), x.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", [8, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_upsample_loss_valid(case, S, dtype):
    from mtlora_amd import functional as Fn
    kind, C, pw = CASES[case]
    low, lab = make_case(kind, C, S, seed=100 * S + C)
    low_q = low.to(dtype)
    lowd, labd = low_q.to(dev()), lab.to(dev())
    vt = 2e-5 if dtype == torch.float32 else 1e-2  # tests/test_gpu_kernels.py::test_upsample_loss_vs_oracle
    gt = 1e-4 if dtype == torch.float32 else 1e-2

    # 1. every sample labelled: the bits of mtlora_upsample_loss fed by mtlora_label_stat
    l_old, g_old = run(kind, lowd, labd, S, pw, None)
    l_one, g_one = run(kind, lowd, labd, S, pw, torch.ones(B, dtype=torch.uint8, device=dev()))
    assert torch.equal(bits(l_old), bits(l_one)), (case, l_old.item(), l_one.item())
    assert torch.equal(bits(g_old), bits(g_one)), case
    assert g_old.dtype == dtype and math.isfinite(l_old.item())

    for name in ("mid", "last"):
        mask = MASKS[name]
        valid = torch.tensor(mask, dtype=torch.uint8, device=dev())
        off = [b for b in range(B) if not mask[b]]
        # 2. against the definition in fp64
        ref_in = low_q.double().requires_grad_(True)
        ref = Fn.upsample_loss_valid_torch(kind, ref_in, lab.double(), S, torch.tensor(mask, dtype=torch.uint8), pos_weight=pw)
        ref.backward()
        loss, grad = run(kind, lowd, labd, S, pw, valid)
        ev = abs(loss.item() - ref.item()) / max(1.0, abs(ref.item()))
        eg = rel_err(grad.float(), ref_in.grad)
        print(case, S, dtype, name, "loss", loss.item(), ref.item(), ev, "d low", eg)
        assert ev <= vt, (case, name, loss.item(), ref.item())
        assert eg <= gt, (case, name, eg)
        # 3. the unlabelled samples' rows are +0.0 ...
        assert int(bits(grad[off]).abs().max()) == 0, (case, name)
        assert float(grad[[b for b in range(B) if mask[b]]].float().abs().max()) > 0.0
        # ... and neither their prediction nor their label is read: any bits there, the same result
        for poison in ("nan", "inf", "ff"):
            lo2, la2 = lowd.clone(), labd.clone()
            for b in off:
                if poison == "ff":
                    lo2[b].view(torch.uint8).fill_(0xFF)
                    la2[b].view(torch.uint8).fill_(0xFF)
                else:
                    lo2[b] = float(poison)
                    la2[b] = float(poison) if poison == "nan" else -float(poison)
            l2, g2 = run(kind, lo2, la2, S, pw, valid)
            assert torch.equal(bits(l2), bits(loss)), (case, name, poison, l2.item(), loss.item())
            assert torch.equal(bits(g2), bits(grad)), (case, name, poison)
        # 5. deterministic
        l3, g3 = run(kind, lowd, labd, S, pw, valid)
        assert torch.equal(bits(l3), bits(loss)) and torch.equal(bits(g3), bits(grad))

    # 4. no labelled sample: +0.0 and all-zero bytes, whatever the inputs hold
    valid = torch.zeros(B, dtype=torch.uint8, device=dev())
    for lo2, la2 in ((lowd, labd), (torch.full_like(lowd, float("nan")), torch.full_like(labd, float("inf")))):
        loss, grad = run(kind, lo2, la2, S, pw, valid)
        assert int(bits(loss.float())) == 0, (case, loss.item())
        assert int(bits(grad).abs().max()) == 0, case


@pytest.mark.parametrize("shape", [(3, 1, 40, 72), (3, 3, 7, 9), (3, 1, 448, 448), (5, 1, 3, 3)], ids=str)
def test_label_stat_valid_against_a_host_count(shape):
    """kind 0 exact; kind 1 the fp32 rounding of the fp64 mean; all labelled: the bits of mtlora_label_stat; the labels of an
    unlabelled sample are not read (NaN there would count as 'not positive' / 'not ignored'); (7, 9) x 3 = 189 values per sample
    is no multiple of 4 (the element walk), 448 x 448 takes 25 blocks per sample"""
    from mtlora_amd import functional as Fn
    n = shape[0]
    g = torch.Generator().manual_seed(sum(shape))
    lab0 = (torch.rand(shape, generator=g) < 0.3).float()
    lab0[torch.rand(shape, generator=g) < 0.1] = 255.0
    masks = [[1] * n, [1, 0] + [1] * (n - 2), [0] * (n - 1) + [1], [0] * n]
    for mask in masks:
        lab = lab0.clone()
        lab[torch.tensor(mask) == 0] = float("nan")
        labd = lab.to(dev())
        valid = torch.tensor(mask, dtype=torch.uint8, device=dev())
        sel = lab0[torch.tensor(mask, dtype=torch.bool)]
        for kind in (0, 1, 2):
            out = Fn.label_stat_valid(labd, valid, kind, 255.0).cpu()
            assert out.shape == (2,) and out[1].item() == float(sum(mask)), (mask, kind, out)
            if kind == 2 or sum(mask) == 0:
                want = 0.0
            elif kind == 0:
                want = float((sel != 255.0).sum().item())
            else:
                want = torch.tensor(float((sel < 0.5).sum().item()) * (1.0 / sel.numel()), dtype=torch.float64).float().item()
            assert out[0].item() == want, (mask, kind, out[0].item(), want)
    labd = lab0.to(dev())
    for kind in (0, 1):
        old = Fn.label_stat(labd, kind, 255.0)
        for valid in (None, torch.ones(n, dtype=torch.uint8, device=dev())):
            new = Fn.label_stat_valid(labd, valid, kind, 255.0)
            assert torch.equal(bits(new[:1]), bits(old)) and new[1].item() == float(n), (kind, new, old)


def test_label_stat_valid_scratch_and_rejects():
    from mtlora_amd import _lib as L
    lib = L.lib()
    lab = torch.zeros(3 * 1000 + 4, device=dev())
    valid = torch.ones(3, dtype=torch.uint8, device=dev())
    out = torch.full((4,), -7.0, device=dev())
    sb = lib.mtlora_label_stat_valid_scratch_bytes(3, 1000)
    assert sb == 3 * 4 + 256 and lib.mtlora_label_stat_valid_scratch_bytes(0, 1000) == -1
    scratch = torch.empty(sb + 16, dtype=torch.uint8, device=dev())
    P = ctypes.c_void_p

    def call(label=lab.data_ptr(), v=valid.data_ptr(), nb=3, n=1000, kind=0, o=out.data_ptr(), s=scratch.data_ptr(), nbytes=sb):
        return lib.mtlora_label_stat_valid(P(label), P(v), nb, n, kind, 255.0, P(o), P(s), nbytes, L.stream_ptr())

    assert call(label=0) == ERR_NULL and call(o=0) == ERR_NULL and call(s=0) == ERR_NULL
    assert call(label=lab.data_ptr() + 4) == ERR_ALIGN and call(s=scratch.data_ptr() + 4) == ERR_ALIGN
    assert call(nb=0) == ERR_SHAPE and call(n=0) == ERR_SHAPE
    assert call(kind=3) == ERR_UNSUPPORTED
    assert call(nbytes=sb - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out == -7.0).all()  # a rejected call launches nothing
    assert call(v=0) == 0 and call(label=0, kind=2) == 0  # NULL flags: all labelled; kind 2 reads no label
    torch.cuda.synchronize()
    assert out[:2].tolist() == [0.0, 3.0] and (out[2:] == -7.0).all()
    with pytest.raises(RuntimeError, match="valid must be a uint8"):
        from mtlora_amd import functional as Fn
        Fn.label_stat_valid(lab[:3000].view(3, 1000), torch.ones(3, device=dev()), 0, 255.0)
    with pytest.raises(RuntimeError, match="contiguous"):  # a strided view would be copied: a replay would not follow the buffer
        Fn.label_stat_valid(lab[:3000].view(3, 1000), torch.ones(6, dtype=torch.uint8, device=dev())[::2], 0, 255.0)


# ------------------------------------------------------------------------------------------------
# model level: the small 2-stage model (56 px, depths (2, 2)), four tasks, B = 3
# ------------------------------------------------------------------------------------------------
TASKS4 = ["semseg", "normals", "sal", "depth"]
MASK4 = {"semseg": [1, 0, 1], "normals": [0, 0, 0], "sal": [0, 1, 1], "depth": [1, 1, 0]}  # normals: wholly unlabelled
MODEL_KW = dict(img_size=56, tasks=TASKS4, depths=(2, 2), num_heads=(3, 6), r_shared=8, r_task=4, drop_path_rate=0.0, seed=4)


def test_train_step_valid_fused_equals_plain():
    """train_step(valid=) with the fused losses against the same model through the un-fused MultiTaskLoss.forward(valid=), fp32,
    dropout off (both passes deterministic, the same forward kernels up to the heads' low-resolution outputs).  Loss and per-task
    losses at 1e-4 (tests/test_gpu_kernels.py::test_fused_loss_path_equals_plain_path); every trainable gradient at the fp32
    tolerance of tests/test_gpu_models.py (1e-3 of the tensor's largest element, floor 1e-6 of the model's largest gradient)."""
    from mtlora_amd import mtl_harness as H
    img, tg, valid = H.synthetic_batch(B, 56, TASKS4, seed=17, device=dev(), valid=MASK4)
    assert torch.isnan(tg["normals"]).all() and torch.isnan(tg["semseg"][1]).all()
    model = H.build_model(**MODEL_KW, DROPOUT=[0.0, 0.0]).to(dev()).train()
    crit, opt = H.MultiTaskLoss(TASKS4), H.build_optimizer(model, lr=1e-3)
    loss, norm = H.train_step(model, crit, opt, img, tg, amp_dtype=None, update_grad=False, valid=valid)
    assert norm is None and math.isfinite(loss.item())
    fused = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    model.zero_grad(set_to_none=True)
    total, per = crit(model(img), tg, valid)
    total.backward()
    plain = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    print("loss", loss.item(), total.item())
    assert abs(loss.item() - total.item()) <= 1e-4 * abs(total.item())
    assert per["normals"].item() == 0.0
    assert set(fused) == set(plain) and len(fused) > 50
    gmax = max(g.abs().max().item() for g in plain.values())
    worst = ("", 0.0)
    for n, r in plain.items():
        assert torch.isfinite(fused[n]).all(), n
        e = (fused[n].double() - r.double()).abs().max().item() / max(r.abs().max().item(), 1e-6 * gmax)
        worst = max(worst, (n, e), key=lambda x: x[1])
        assert e <= 1e-3, (n, e)
    print("worst gradient", worst)
    # the wholly unlabelled task: its head and its task-specific factors got zero gradients, not NaN
    own = [n for n in fused if ".normals." in n or n.endswith(".normals") or "_normals" in n]
    assert any("decoders" in n for n in own), own
    for n in own:
        assert float(fused[n].abs().max()) == 0.0, n
    assert any(float(fused[n].abs().max()) > 0.0 for n in fused if "semseg" in n)


def test_graphed_train_step_follows_the_valid_buffers():
    """GraphedTrainStep(valid=): ONE capture, the masks written into the static buffers between replays.  Each call against an
    eager train_step(valid=) from the same state with the same dropout seeds; criterion of
    tests/test_gpu_linear_bias.py::test_graphed_train_step_with_bias_all (losses and gradient norms within 2e-3 relative, cosine of
    the accumulated updates >= 0.98).  With every flag 0 the replayed loss is exactly 0."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    other = {"semseg": [0, 1, 1], "normals": [1, 1, 0], "sal": [0, 0, 0], "depth": [1, 0, 1]}
    zero = {t: [0, 0, 0] for t in TASKS4}
    img, tg = H.synthetic_batch(B, 56, TASKS4, seed=17, device=dev())
    out = []
    for use_graph in (True, False):
        torch.manual_seed(9)
        Fn._seed_counter = 0
        model = H.build_model(**MODEL_KW).to(dev()).train()
        crit, opt = H.MultiTaskLoss(TASKS4), H.build_optimizer(model, lr=1e-3, impl="hip", capturable=True)
        vbuf = {t: torch.tensor(MASK4[t], dtype=torch.uint8, device=dev()) for t in TASKS4}
        try:
            gs = H.GraphedTrainStep(model, crit, opt, img, tg, clip_grad=5.0, warmup=2, valid=vbuf)
            assert gs.graphed is True and gs.why == "", gs.why
            graph = gs.g_bwd
            drawn = Fn._seed_counter
            assert drawn % 3 == 0
            start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
            losses, norms = [], []
            for masks in (MASK4, other, zero, MASK4):
                for t in TASKS4:
                    vbuf[t].copy_(torch.tensor(masks[t], dtype=torch.uint8))
                if use_graph:
                    loss, norm = gs(), gs.grad_norm
                else:
                    Fn._seed_counter = 2 * drawn // 3
                    gs.seed.add_(gs.SEED_STEP)
                    loss, norm = H.train_step(model, crit, opt, img, tg, clip_grad=5.0, valid=vbuf)
                losses.append(loss.clone())
                norms.append(norm.clone())
            torch.cuda.synchronize()
            assert gs.graphed is True and gs.g_bwd is graph  # no re-capture
            out.append((losses, {n: (p.detach() - start[n]).double() for n, p in model.named_parameters() if n in start}, norms))
        finally:
            Fn.set_seed_offset(None)
    for i, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        print("loss", i, a.item(), b.item())
        assert math.isfinite(a.item()) and abs(a.item() - b.item()) <= 2e-3 * abs(b.item()), (i, a.item(), b.item())
    assert out[0][0][2].item() == 0.0 and out[1][0][2].item() == 0.0  # every flag 0
    assert out[0][0][0].item() != out[0][0][1].item()
    for i, (a, b) in enumerate(zip(out[0][2], out[1][2])):
        print("grad norm", i, a.item(), b.item())
        assert math.isfinite(a.item()) and abs(a.item() - b.item()) <= 2e-3 * abs(b.item()) + 1e-12, (i, a.item(), b.item())
    num = sum((out[0][1][n] * out[1][1][n]).sum().item() for n in out[0][1])
    den = (sum((out[0][1][n] ** 2).sum().item() for n in out[0][1]) * sum((out[1][1][n] ** 2).sum().item() for n in out[1][1])) ** 0.5
    print("cosine", num / den)
    assert num / den >= 0.98, num / den


def test_graphed_train_step_valid_needs_the_fused_loss():
    from mtlora_amd import mtl_harness as H
    with pytest.raises(ValueError, match="fused_loss"):
        H.GraphedTrainStep(None, None, None, torch.zeros(1, device=dev()), {}, fused_loss=False,
                           valid={"semseg": torch.ones(1, dtype=torch.uint8, device=dev())})
    with pytest.raises(ValueError, match="no fused loss kind"):
        H.GraphedTrainStep(None, None, None, torch.zeros(1, device=dev()), {}, valid={"flow": torch.ones(1, dtype=torch.uint8, device=dev())})


def test_prepare_batch_of_a_merged_wire_batch():
    """PASCAL-Context + NYUD in one wire batch: prepare_batch on the GPU equals prepare_batch_torch bit for bit on the labelled
    samples, and both hand the flags through; the loss of the merged batch never reads the undefined planes"""
    from mtlora_amd import data as D
    from mtlora_amd import mtl_harness as H
    pascal = ["semseg", "human_parts", "sal", "normals", "edge"]
    a = D.synthetic_wire_batch(2, 16, pascal, seed=3)
    b = D.synthetic_wire_batch(1, 16, list(H.NYUD4), seed=4, num_outputs=H.NYUD_NUM_OUTPUT)
    m, tasks = D.merge_wire_batches(a, pascal, b, H.NYUD4)
    for t in tasks:  # make the undefined planes defined for the comparison of the run itself: garbage both sides agree on
        off = m["valid"][t] == 0
        if off.any():
            m[t][off] = 255 if m[t].dtype == torch.uint8 else float("nan")
    md = {k: ({t: v.to(dev()) for t, v in x.items()} if k == "valid" else x.to(dev())) for k, x in m.items()}
    assert len(D.prepare_batch({k: v for k, v in md.items() if k != "valid"}, tasks)) == 2
    images, targets, valid = D.prepare_batch(md, tasks)
    ri, rt, rv = D.prepare_batch_torch(m, tasks)
    assert torch.equal(images.cpu(), ri)
    for t in tasks:
        on = m["valid"][t] != 0
        assert valid[t].is_cuda and valid[t].dtype == torch.uint8 and torch.equal(valid[t].cpu(), rv[t]) and torch.equal(rv[t], m["valid"][t])
        assert torch.equal(bits(targets[t][on.to(dev())]), bits(rt[t][on])), t
    assert valid["depth"].tolist() == [0, 0, 1] and valid["human_parts"].tolist() == [1, 1, 0]
    # the flags go straight into the fused loss
    crit = H.MultiTaskLoss(["depth", "sal"])
    low = {"depth": torch.randn(3, 4, 4, 1, device=dev()), "sal": torch.randn(3, 4, 4, 1, device=dev())}
    total, per = crit.forward_low(low, targets, valid)
    assert math.isfinite(total.item()) and per["depth"].item() > 0.0
