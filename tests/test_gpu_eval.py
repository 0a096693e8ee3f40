"""GPU tests of the validation path: csrc/metrics.hip (through the C ABI), the l1_masked / edge kinds of csrc/loss.hip,
PerformanceMeter.update_low and mtl_harness.validate_step / validate.

The expected values are an fp64 restatement written HERE (the oracle has no metrics): the same (dtype-rounded) low-resolution
tensor, upcast, F.interpolate in fp64 on the CPU, then the meters' formulas.  Only the kernel's fp32 arithmetic differs, so

* a DECISION (argmax, a threshold on the probability, a degree bin) can differ only for a pixel that sits on the boundary.  The
  fp64 side marks a pixel ambiguous for a decision when its margin to the boundary is below
  delta = 16 fp32 ulps of the largest |interpolated value| of the tensor (3 fma of the bilinear blend, then sigmoid / normalise,
  rounded up generously).  For the degree bins the compared quantity is an angle in degrees (up to 180, behind acos, whose
  slope at the 11.25-degree bin is 5), so the margin there is taken in degrees against 16 fp32 ulps of 180 (2.4e-4 degrees).
  Every count must satisfy |kernel - reference| <= number of ambiguous pixels feeding that count, and the inputs must keep the
  ambiguous share (union over the kind's decisions) at or below 1e-3 of the pixels -- a condition on the inputs, checked on
  the fp64 side alone.
  The depth meter's clamp max(p, 1e-9) makes log p discontinuous at p = 0: the inputs must have no valid pixel with
  |interpolated value| < 1e-4 (asserted on the fp64 side).
* FLOAT sums (degree sums, depth squares, the loss values): relative error against fp64 at most 1e-5.

Measured on MI355X (profiles/eval_gpu_tests.txt, every figure of every case): the largest relative error of a float sum over
all cases of this file is 1.5e-7 (the edge meter's loss, 4 x 33 x 70 at scale 1; the bound is 1e-5); the largest ambiguous
share of the inputs is 8.8e-4 (semseg-40, bf16, 2 x 21 x 27 at scale 3; fp32 inputs: at most 6e-4, the saliency kind's 34
thresholds); the largest count difference is 4 pixels of 401 408 (semseg, bf16 input, 5 ambiguous), with fp32 inputs 1 pixel.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-5
AMBIGUOUS_SHARE = 1e-3
KIND_OF = {"semseg": "softmax", "human_parts": "softmax", "semseg40": "softmax", "normals": "normals", "sal": "saliency",
           "depth": "l1_masked", "edge": "edge"}
CH = {"semseg": 21, "human_parts": 7, "semseg40": 40, "normals": 3, "sal": 1, "depth": 1, "edge": 1}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def make_case(task, B, h, w, S, seed):
    g = torch.Generator().manual_seed(seed)
    C, H, W = CH[task], h * S, w * S
    if task in ("semseg", "human_parts", "semseg40"):
        low = torch.randn(B, h, w, C, generator=g)
        lab = torch.randint(0, C, (B, 1, H, W), generator=g).float()
        lab[torch.rand(B, 1, H, W, generator=g) < 0.07] = 255.0
    elif task == "normals":
        low = torch.randn(B, h, w, C, generator=g)
        lab = F.normalize(torch.randn(B, 3, H, W, generator=g), dim=1)
        lab[torch.rand(B, 3, H, W, generator=g) < 0.03] = 255.0
    elif task == "sal":
        low = torch.randn(B, h, w, C, generator=g)
        lab = (torch.rand(B, 1, H, W, generator=g) < 0.3).float()
        lab[torch.rand(B, 1, H, W, generator=g) < 0.03] = 255.0
        if B > 1:
            lab[-1] = 0.0  # an image without a positive pixel
    elif task == "depth":
        low = 3.0 + 0.8 * torch.randn(B, h, w, C, generator=g)
        lab = 0.5 + 9 * torch.rand(B, 1, H, W, generator=g)
        lab[torch.rand(B, 1, H, W, generator=g) < 0.07] = 255.0
    else:
        low = torch.randn(B, h, w, C, generator=g) - 1.0
        lab = (torch.rand(B, 1, H, W, generator=g) < 0.1).float()
    return low, lab


def sal_thresholds():
    from mtlora_amd import functional as Fn
    t = Fn.saliency_thresholds().double()
    return t[:15], t[15:]


def reference(task, low_q, lab, S):
    """fp64 restatement.  Returns counts / ambiguous (kernel layout, int64 arrays), sums (loss first), ambiguous pixel share."""
    kind = KIND_OF[task]
    up = F.interpolate(low_q.double().permute(0, 3, 1, 2), scale_factor=S, mode="bilinear")
    lab = lab.double()
    B, C, H, W = up.shape
    npix = B * H * W
    delta = 16.0 * float(np.spacing(np.float32(up.abs().max().item())))
    if kind == "softmax":
        valid = lab[:, 0] != 255
        top = up.topk(2, dim=1)
        am, second = top.indices[:, 0], top.indices[:, 1]
        amb = (top.values[:, 0] - top.values[:, 1] < delta) & valid
        gt = lab[:, 0].long()
        cnt, ab = np.zeros(3 * C + 1, np.int64), np.zeros(3 * C + 1, np.int64)
        for c in range(C):
            cnt[c] = ((am == c) & (gt == c) & valid).sum()
            cnt[C + c] = ((am == c) & valid).sum()
            cnt[2 * C + c] = ((gt == c) & valid).sum()
            ab[c] = (amb & (gt == c)).sum()
            ab[C + c] = (amb & ((am == c) | (second == c))).sum()
        cnt[3 * C] = valid.sum()
        loss = F.cross_entropy(up, torch.where(valid, gt, torch.full_like(gt, 255)), ignore_index=255)
        return cnt, ab, [loss.item()], amb.sum().item() / npix
    if kind == "normals":
        ok = lab != 255
        n = up / (up.norm(dim=1, keepdim=True) + 1e-12)
        p = 2 * ((n + 1.0) * 255 / 2.0) / 255 - 1
        z = torch.zeros_like(p)
        d1 = (180 / math.pi) * torch.acos(torch.clamp((torch.where(ok, p, z) * torch.where(ok, lab, z)).sum(1), -1, 1))
        m1 = ok[:, 0]
        unit = lambda x: x / x.norm(dim=1, keepdim=True).clamp_min(1e-300)
        pn, gn = unit(p), unit(lab)
        d2 = torch.rad2deg(2 * torch.atan2((pn - gn).norm(dim=1), (pn + gn).norm(dim=1)))
        m2 = ok.all(1)
        ddeg = 16.0 * float(np.spacing(np.float32(180.0)))
        cnt, ab = np.zeros(5, np.int64), np.zeros(5, np.int64)
        cnt[0], cnt[4] = m1.sum(), m2.sum()
        union = torch.zeros_like(m1)
        for i, thr in enumerate((11.25, 22.5, 30.0)):
            cnt[1 + i] = (m1 & (d1 < thr)).sum()
            a = m1 & ((d1 - thr).abs() < ddeg)
            ab[1 + i] = a.sum()
            union |= a
        loss = ((n - lab).abs() * ok).sum() / ok.sum().clamp_min(1e-6)
        return cnt, ab, [loss.item(), d1[m1].sum().item(), d2[m2].sum().item()], union.sum().item() / npix
    o, l = up[:, 0], lab[:, 0]
    if kind in ("saliency", "edge"):
        labels = (l >= 0.5).double()
        w = (1.0 - labels).sum() / labels.numel() if kind == "saliency" else 0.95

        def bce(x):
            gz = (x >= 0).double()
            lv = x * (labels - gz) - torch.log(1 + torch.exp(x - 2 * x * gz))
            return ((w * (-(labels * lv)).sum() + (1 - w) * (-((1.0 - labels) * lv)).sum()) / labels.numel()).item()

        p = torch.sigmoid(o)
        if kind == "edge":
            return np.zeros(0, np.int64), np.zeros(0, np.int64), [bce(o), bce(p)], 0.0
        t1, t2 = sal_thresholds()
        cnt, ab = np.zeros(57 + 45 * B, np.int64), np.zeros(57 + 45 * B, np.int64)
        gpos, valid = l != 0, l != 255
        tg = torch.where(valid, l.long(), torch.zeros_like(l, dtype=torch.long))
        q = torch.sigmoid(p)
        union = torch.zeros_like(gpos)
        for j, t in enumerate(t2.tolist()):
            f, a = (q >= t) & valid, ((q - t).abs() < delta) & valid
            cnt[3 * j:3 * j + 3] = [(f * tg).sum(), f.sum(), tg.sum()]
            ab[3 * j:3 * j + 3] = [(a * tg).sum(), a.sum(), 0]
            union |= a
        for j, t in enumerate(t1.tolist()):
            m, a = p > t, (p - t).abs() < delta
            union |= a
            for b in range(B):
                at = 57 + (b * 15 + j) * 3
                tp = (m[b] & gpos[b]).sum()
                cnt[at:at + 3] = [tp, m[b].sum() - tp, gpos[b].sum() - tp]
                ab[at:at + 3] = [(a[b] & gpos[b]).sum(), (a[b] & ~gpos[b]).sum(), (a[b] & gpos[b]).sum()]
        return cnt, ab, [bce(o)], union.sum().item() / npix
    # depth
    valid = l != 255
    assert int(((o.abs() < 1e-4) & valid).sum()) == 0, "input condition: no valid pixel at the clamp's discontinuity"
    pc = o.clamp_min(1e-9)
    loss = ((o - l).abs() * valid).sum() / valid.sum().clamp_min(1.0)
    sq, lsq = ((l - pc) ** 2)[valid].sum(), ((torch.log(l) - torch.log(pc)) ** 2)[valid].sum()
    return np.array([valid.sum().item()], np.int64), np.zeros(1, np.int64), [loss.item(), sq.item(), lsq.item()], 0.0


def check(what, counts, sums, ref):
    cnt, ab, rsums, share = ref
    print(f"{what}: ambiguous share {share:.3e}")
    assert share <= AMBIGUOUS_SHARE, (what, share)
    got = np.asarray(counts, np.int64)[:len(cnt)]
    diff = np.abs(got - cnt)
    print(f"{what}: max |count - ref| {int(diff.max()) if len(diff) else 0}, ambiguous max {int(ab.max()) if len(ab) else 0}")
    assert (diff <= ab).all(), (what, np.nonzero(diff > ab)[0][:8], got[diff > ab][:8], cnt[diff > ab][:8], ab[diff > ab][:8])
    worst = 0.0
    for i, (a, b) in enumerate(zip(sums, rsums)):
        e = abs(float(a) - b) / max(abs(b), 1e-300)
        worst = max(worst, e)
        print(f"{what}: float sum {i} kernel {float(a):.9g} fp64 {b:.9g} rel {e:.3e}")
    assert worst <= FLOAT_RTOL, (what, worst)
    return worst


GEOM = [(2, 56, 56, 8),   # the heads' geometry
        (2, 26, 30, 4),   # non-square, scale 4, width not a multiple of the 16-column tile, a partial last row tile
        (4, 33, 70, 1),   # scale 1 (64-column tiles, 70 columns)
        (1, 10, 21, 8),   # width not a multiple of the 8-column tile, a partial last row tile
        (2, 21, 27, 3)]   # 63 of the 64 lanes carry a column
# (maps of a few thousand pixels at least: the saliency kind's 34 thresholds put about 3e-4 of N(0, 1) pixels within delta of one,
#  on a map of a thousand pixels one such pixel is already 1e-3)


def quantise(low, dtype):
    """the low-resolution tensor in the kernel's input dtype.  bf16 keeps 8 bits, so two of C random logits of a pixel tie
    EXACTLY for about 1 pixel in 100; where the interpolation copies a source pixel (scale 1, clamped borders) that tie
    survives and is a margin of 0.  Such inputs do not meet the ambiguity condition whatever the seed, so the winner of a
    tied low-resolution pixel is moved up by two bf16 steps."""
    q = low.to(dtype)
    if dtype == torch.bfloat16 and low.shape[-1] > 4:
        f = q.float()
        top = f.topk(2, dim=-1)
        tie = top.values[..., 0] == top.values[..., 1]
        bumped = top.values[..., 0] + top.values[..., 0].abs().clamp_min(0.01) * 2.0 ** -6
        f.scatter_(-1, top.indices[..., :1], torch.where(tie, bumped, top.values[..., 0]).unsqueeze(-1))
        q = f.to(dtype)
    return q


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,h,w,S", GEOM)
@pytest.mark.parametrize("task", ["semseg", "human_parts", "semseg40", "normals", "sal", "depth", "edge"])
def test_metrics_kernel_vs_fp64(task, B, h, w, S, dtype):
    """mtlora_upsample_metrics against the fp64 restatement: counts within the ambiguous pixels, float sums to 1e-5."""
    from mtlora_amd import functional as Fn
    low, lab = make_case(task, B, h, w, S, seed=7 * h + w + S)
    low_q = quantise(low, dtype)
    ref = reference(task, low_q, lab, S)
    counts, sums = Fn.upsample_metrics(KIND_OF[task], low_q.to(dev()), lab.to(dev()), S)
    check(f"{task} {B}x{h}x{w} S{S} {dtype}", counts.cpu().numpy(), sums.cpu().tolist(), ref)
    # counts are ADDED to: a second launch into the same array doubles them
    if len(ref[0]):
        c2, _ = Fn.upsample_metrics(KIND_OF[task], low_q.to(dev()), lab.to(dev()), S, counts=counts.clone())
        assert torch.equal(c2, 2 * counts)


def test_metrics_sizes_and_validation():
    import ctypes
    from mtlora_amd import _lib
    L = _lib.lib()
    ni, nf = ctypes.c_int64(), ctypes.c_int64()
    assert L.mtlora_upsample_metrics_sizes(0, 2, 56, 56, 21, 8, ctypes.byref(ni), ctypes.byref(nf)) == 0
    assert ni.value == 64 and nf.value == 2 * 14 * 7
    assert L.mtlora_upsample_metrics_sizes(2, 3, 8, 8, 1, 4, ctypes.byref(ni), ctypes.byref(nf)) == 0 and ni.value == 57 + 45 * 3
    assert L.mtlora_upsample_metrics_sizes(0, 2, 8, 8, 49, 4, ctypes.byref(ni), ctypes.byref(nf)) < 0
    assert L.mtlora_upsample_metrics_sizes(1, 2, 8, 8, 5, 4, ctypes.byref(ni), ctypes.byref(nf)) < 0
    assert L.mtlora_upsample_metrics_sizes(3, 2, 8, 8, 2, 4, ctypes.byref(ni), ctypes.byref(nf)) < 0
    assert L.mtlora_upsample_metrics_sizes(0, 2, 8, 8, 21, 33, ctypes.byref(ni), ctypes.byref(nf)) < 0
    assert L.mtlora_upsample_metrics_sizes(5, 2, 8, 8, 1, 4, ctypes.byref(ni), ctypes.byref(nf)) < 0
    assert L.mtlora_upsample_metrics(0, None, None, None, None, None, 2, 8, 8, 21, 4, _lib.F32, 255.0, None) == -4
    assert L.mtlora_upsample_metrics(0, None, None, None, None, None, 2, 8, 8, 21, 4, _lib.F16, 255.0, None) == -1


ALL6 = ["semseg", "human_parts", "normals", "sal", "depth", "edge"]


def _meter_state(meter, task):
    """(counts in the kernel's layout, float sums without the loss) of one task's meter"""
    m = meter.meters[task]
    c = m.counts.cpu().numpy()
    if task == "sal":
        c = np.concatenate([c[:57], torch.cat(m.per_image).cpu().numpy().reshape(-1)])
    if task == "edge":
        return np.zeros(0, np.int64), [m.sums[0].item() / m.n]
    s = m.sums.cpu().tolist()
    return c, (s if task in ("normals", "depth") else [])


def _ref_accumulate(refs, task):
    """the fp64 restatement accumulated over batches the way a meter accumulates"""
    if task == "sal":
        cnt = np.concatenate([sum(r[0][:57] for r in refs)] + [r[0][57:] for r in refs])
        ab = np.concatenate([sum(r[1][:57] for r in refs)] + [r[1][57:] for r in refs])
    else:
        cnt, ab = sum(r[0] for r in refs), sum(r[1] for r in refs)
    if task == "edge":
        sums = [sum(r[2][1] for r in refs) / len(refs)]  # equal batch sizes: numel-weighted mean == mean
    else:
        sums = [sum(r[2][i] for r in refs) for i in range(1, len(refs[0][2]))]
    return cnt, ab, [0.0] + sums, max(r[3] for r in refs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_update_low_vs_update_on_full_resolution(dtype):
    """PerformanceMeter.update_low (fused) and update(get_output(F.interpolate(...))) (plain torch on the same GPU) over three
    batches: BOTH meter states are held to the fp64 restatement by the bound of test_metrics_kernel_vs_fp64, and the
    losses update_low returns to 1e-5."""
    from mtlora_amd.evaluation import PerformanceMeter, get_output
    B, h, w, S = 2, 28, 28, 8
    fused, plain = PerformanceMeter(ALL6), PerformanceMeter(ALL6)
    refs = {t: [] for t in ALL6}
    for i in range(3):
        low, lab = {}, {}
        for k, t in enumerate(ALL6):
            lo, lab[t] = make_case(t, B, h, w, S, seed=100 * i + k)
            low[t] = quantise(lo, dtype)
            refs[t].append(reference(t, low[t], lab[t], S))
        lowd, labd = {t: v.to(dev()) for t, v in low.items()}, {t: v.to(dev()) for t, v in lab.items()}
        losses = fused.update_low(lowd, labd)
        for t in ALL6:
            e = abs(losses[t].item() - refs[t][-1][2][0]) / abs(refs[t][-1][2][0])
            print(f"batch {i} {t}: loss rel err {e:.3e}")
            assert e <= FLOAT_RTOL, (t, e)
        up = {t: F.interpolate(lowd[t].float().permute(0, 3, 1, 2), scale_factor=S, mode="bilinear") for t in ALL6}
        plain.update({t: get_output(up[t], t) for t in ALL6}, labd)
    for t in ALL6:
        ref = _ref_accumulate(refs[t], t)
        for name, meter in (("fused", fused), ("plain", plain)):
            c, s = _meter_state(meter, t)
            check(f"{name} {t} {dtype}", c, [0.0] + s, (ref[0], ref[1], ref[2], ref[3]))
    sf, sp = fused.get_score(verbose=False), plain.get_score(verbose=False)
    assert set(sf) == set(sp) == set(ALL6)
    for t in ALL6:
        assert set(sf[t]) == set(sp[t])


# ------------------------------------------------------------------------------------------------
# training side: the l1_masked kind and edge (balanced_bce with the constant weight)
# ------------------------------------------------------------------------------------------------
def _ref_loss(task, up, lab):
    if task == "depth":  # DepthLoss: L1 over label != 255, mean over the valid pixels
        mask = lab != 255
        return ((up - lab).abs() * mask).sum() / mask.sum()
    labels = (lab >= 0.5).double()  # BalancedCrossEntropyLoss(size_average, pos_weight=0.95)
    gz = (up >= 0).double()
    lv = up * (labels - gz) - torch.log(1 + torch.exp(up - 2 * up * gz))
    return (0.95 * (-(labels * lv)).sum() + 0.05 * (-((1.0 - labels) * lv)).sum()) / labels.numel()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("task,B,h,w,S", [("depth", 2, 20, 20, 4), ("edge", 3, 18, 33, 4), ("depth", 2, 37, 16, 4), ("edge", 1, 7, 9, 2),
                                          ("depth", 2, 5, 40, 3), ("edge", 1, 16, 16, 1), ("depth", 2, 28, 28, 8), ("edge", 2, 28, 28, 8),
                                          ("depth", 1, 14, 21, 8), ("edge", 3, 9, 70, 1), ("depth", 2, 6, 5, 16), ("edge", 1, 5, 4, 32),
                                          ("depth", 5, 13, 15, 8), ("edge", 2, 9, 23, 3), ("depth", 1, 16, 16, 1), ("edge", 2, 6, 5, 16)])
def test_upsample_loss_l1_masked_and_edge_vs_fp64(task, B, h, w, S, dtype):
    """value and d low of the two new fused training losses against DepthLoss / BalancedCrossEntropyLoss(pos_weight=0.95) on
    torch's fp64 bilinear upsample (CPU); tolerances of test_upsample_loss_vs_oracle."""
    from mtlora_amd import functional as Fn
    from mtlora_amd.mtl_harness import MultiTaskLoss
    low, lab = make_case(task, B, h, w, S, seed=h * 100 + w)
    low_q = low.to(dtype)
    ref_in = low_q.double().requires_grad_(True)
    up = F.interpolate(ref_in.permute(0, 3, 1, 2), scale_factor=S, mode="bilinear")
    ref = _ref_loss(task, up, lab.double())
    ref.backward()
    x = low_q.to(dev()).requires_grad_(True)
    crit = MultiTaskLoss([task])
    got = crit.task_low(task, x, lab.to(dev()))
    assert got.grad_fn is not None and type(got.grad_fn).__name__.startswith("UpsampleLossFn")
    (got * 3.0).backward()
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    print(task, got.item(), ref.item(), abs(got.item() - ref.item()) / max(1.0, abs(ref.item())))
    assert abs(got.item() - ref.item()) <= tol * max(1.0, abs(ref.item())), (got.item(), ref.item())
    e = rel_err(x.grad.float() / 3.0, ref_in.grad)
    print(task, "d low", e)
    assert e <= (1e-4 if dtype == torch.float32 else 1e-2), e
    assert Fn.LOSS_KINDS["l1_masked"] == 3


def test_fused_loss_path_equals_plain_path_nyud():
    """MultiTaskLoss.forward_low(low) == MultiTaskLoss.forward(F.interpolate(low)) for the NYUD task set (semseg-40, depth,
    normals, edge): value and gradient at 1e-4."""
    from mtlora_amd import mtl_harness as H
    tasks = list(H.NYUD4)
    crit = H.MultiTaskLoss(tasks)
    low, gt = {}, {}
    for i, t in enumerate(tasks):
        lo, lab = make_case("semseg40" if t == "semseg" else t, 2, 24, 24, 4, seed=i)
        low[t], gt[t] = (2 * lo).to(dev()).requires_grad_(True), lab.to(dev())
    total, per = crit.forward_low(low, gt)
    total.backward()
    g_fused = {t: low[t].grad.clone() for t in tasks}
    for t in tasks:
        low[t].grad = None
    pred = {t: F.interpolate(low[t].permute(0, 3, 1, 2), scale_factor=4, mode="bilinear") for t in tasks}
    total2, per2 = crit(pred, gt)
    total2.backward()
    assert abs(total.item() - total2.item()) <= 1e-4 * abs(total2.item())
    for t in tasks:
        assert abs(per[t].item() - per2[t].item()) <= 1e-4 * max(1.0, abs(per2[t].item())), t
        assert rel_err(g_fused[t], low[t].grad) <= 1e-4, t


def _small(tasks, num_outputs=None, seed=0):
    from mtlora_amd import mtl_harness as H
    return H.build_model(img_size=224, tasks=tasks, r_shared=16, r_task=4, seed=seed, num_outputs=num_outputs).to(dev())


def test_train_step_nyud_task_set():
    from mtlora_amd import mtl_harness as H
    model = _small(H.NYUD4, H.NYUD_NUM_OUTPUT).train()
    assert model.decoders.decoders["semseg"].last_layer[3].out_channels == 40
    crit, opt = H.MultiTaskLoss(model.tasks), H.build_optimizer(model, lr=1e-4)
    img, tg = H.synthetic_batch(2, 224, model.tasks, seed=1, device=dev(), num_outputs=H.NYUD_NUM_OUTPUT)
    loss, norm = H.train_step(model, crit, opt, img, tg, fused_loss=True)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(norm), (loss, norm)


# ------------------------------------------------------------------------------------------------
# validate_step / validate
# ------------------------------------------------------------------------------------------------
def _warm_bn(model, tasks, num_outputs=None):
    """a few train-mode forwards so that the BatchNorm running statistics are not the initial ones"""
    from mtlora_amd import mtl_harness as H
    model.train()
    with torch.no_grad():
        for s in range(2):
            img, _ = H.synthetic_batch(2, 224, tasks, seed=50 + s, device=dev(), num_outputs=num_outputs)
            model(img, upsample=False)
    return model


@pytest.mark.parametrize("tasks", [("semseg", "normals", "sal", "human_parts"), tuple(ALL6)], ids=["pascal4", "all6"])
def test_validate_step_vs_full_resolution_route(tasks):
    """validate_step (fused) against model(images) -> get_output -> torch meters on the same GPU, fp32: both meter states within
    the bound of test_metrics_kernel_vs_fp64 of the fp64 restatement on the model's own low-resolution outputs; parameters,
    buffers and the training flag unchanged."""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import PerformanceMeter, get_output
    model = _warm_bn(_small(tasks), tasks)
    if "depth" in tasks:  # input condition of the depth meter (see the module docstring): predictions away from the clamp at 0
        with torch.no_grad():
            model.decoders.decoders["depth"].last_layer[3].bias.fill_(3.0)
    crit = H.MultiTaskLoss(tasks)
    before = {k: v.detach().clone() for k, v in list(model.named_parameters()) + list(model.named_buffers())}
    fused, plain = PerformanceMeter(tasks), PerformanceMeter(tasks)
    refs = {t: [] for t in tasks}
    assert model.training
    for i in range(2):
        img, tg = H.synthetic_batch(2, 224, tasks, seed=10 + i, device=dev())
        if "sal" in tasks:
            tg["sal"][-1] = 0.0
        total, per = H.validate_step(model, crit, fused, img, tg, amp_dtype=None)
        assert model.training and total.is_cuda and set(per) == set(tasks) | {"total"}
        model.eval()
        with torch.no_grad():
            full = model(img)
            low = model(img, upsample=False)
            total2, per2 = crit(full, tg)
        model.train()
        plain.update({t: get_output(full[t], t) for t in tasks}, tg)
        assert abs(total.item() - total2.item()) <= 1e-4 * abs(total2.item()), (total.item(), total2.item())
        for t in tasks:
            refs[t].append(reference(t, low[t].cpu(), tg[t].cpu(), 8))
    after = {k: v for k, v in list(model.named_parameters()) + list(model.named_buffers())}
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for t in tasks:
        ref = _ref_accumulate(refs[t], t)
        for name, meter in (("fused", fused), ("plain", plain)):
            c, s = _meter_state(meter, t)
            check(f"validate_step {name} {t}", c, [0.0] + s, ref)
    sf, sp = fused.get_score(verbose=False), plain.get_score(verbose=False)
    for t in tasks:
        assert set(sf[t]) == set(sp[t]), t


def test_validate_merged_equals_unmerged_and_is_deterministic():
    """validate() on a merged model scores as the unmerged one (tolerance of test_merge_matches_unmerged_eval: 1e-3 relative in
    fp32), two identical runs give bit-identical counters and float sums, and the training flag is restored."""
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.checkpoint import merge_lora_weights, unmerge_lora_weights
    from mtlora_amd.evaluation import PerformanceMeter
    tasks = ("semseg", "normals", "sal", "human_parts")
    model = _warm_bn(_small(tasks), tasks).eval()
    batches = [H.synthetic_batch(2, 224, tasks, seed=20 + i, device=dev()) for i in range(2)]

    def run(amp):
        meter = PerformanceMeter(tasks)
        scores, loss = H.validate(model, batches, meter=meter, amp_dtype=amp)
        state = {t: (meter.meters[t].counts.clone(), meter.meters[t].sums.clone()) for t in tasks}
        state["sal_img"] = (torch.cat(meter.meters["sal"].per_image), torch.zeros(1))
        return scores, loss, state

    for amp in (None, torch.bfloat16):
        s1, l1, st1 = run(amp)
        s2, l2, st2 = run(amp)
        assert l1 == l2 and not model.training
        for k in st1:
            assert torch.equal(st1[k][0], st2[k][0]) and torch.equal(st1[k][1], st2[k][1]), (amp, k)
    s_un, l_un, _ = run(None)
    assert merge_lora_weights(model.backbone) > 0
    try:
        s_m, l_m, _ = run(None)
    finally:
        unmerge_lora_weights(model.backbone)
    assert abs(l_m - l_un) <= 1e-3 * abs(l_un), (l_m, l_un)
    for t in tasks:
        for k, v in s_un[t].items():
            a, b = np.asarray(s_m[t][k], float), np.asarray(v, float)
            print(t, k, float(np.abs(a - b).max()))
            assert np.all(np.abs(a - b) <= 1e-3 * np.maximum(1.0, np.abs(b))), (t, k, a, b)
    model.train()
    H.validate(model, batches[:1], amp_dtype=None)
    assert model.training
