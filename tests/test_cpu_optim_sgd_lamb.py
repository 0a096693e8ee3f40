"""Host side of FusedSGD / FusedLAMB (mtlora_amd/optim.py, csrc/optim.hip): the portable definitions ``sgd_update_torch`` and
``lamb_update_torch`` (what the kernels compute, stated in plain torch), the constructors' rejections, ``build_optimizer(name=)``
and the header / ctypes agreement of the four new exports.  No GPU.

This file also owns the tensor set, the fp64 references and the error measures that tests/test_gpu_optim_sgd_lamb.py runs the
kernels against, and ``test_fp32_standins_against_fp64`` measures what an fp32 stand-in for the kernels (torch.optim.SGD in fp32;
lamb_update_torch in fp32) shows against those references on exactly these inputs: the figures the GPU file's bounds come from."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the tensor set (tests/test_gpu_optim.py's: below, at, one past and several times the 4096-element chunk) ---------------------
SHAPES = [(1,), (3,), (64,), (1023,), (4096,), (4097,), (3 * 4096 + 5,), (37, 129)]
ZERO_SHAPE = (4100,)  # LAMB only: an all-zero parameter in the decay group (|p| = 0: ratio = lr)
LR, WD, MAX_NORM = 1e-2, 0.05, 5.0
MOMENTUM = 0.9
BETAS, LAMB_EPS, MAX_GRAD_NORM = (0.9, 0.999), 1e-6, 1.0
GRAD_SCALES = (1e-7, 0.01, 30.0)  # norms ~1.6e-5, ~1.6, ~4.8e3: max_norm idle, idle, active; LAMB's max_grad_norm idle, active, active

_FIGURES = []


def fig(what, value):
    _FIGURES.append(f"{what}: {value:.3e}")
    print(_FIGURES[-1])


def write_figures(figures):
    path = os.environ.get("MTLORA_OPTIM_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(figures) + "\n")


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    write_figures(_FIGURES)


def decays(shape):
    n = int(np.prod(shape))
    return n >= 4096 or len(shape) == 2


def common_inputs(shapes=SHAPES, scales=GRAD_SCALES, seed=0, zero=()):
    """(initial values, per-step gradients): fp32 CPU tensors from one seeded generator; the shapes in ``zero`` start at 0"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in shapes]
    for i, s in enumerate(shapes):
        if s in zero:
            init[i].zero_()
    grads = [[torch.randn(s, generator=g) * sc for s in shapes] for sc in scales]
    return init, grads


def groups_of(params, shapes=SHAPES):
    return [{"params": [p for p, s in zip(params, shapes) if decays(s)]},
            {"params": [p for p, s in zip(params, shapes) if not decays(s)], "weight_decay": 0.0}]


def group_index(shapes=SHAPES):
    return [0 if decays(s) else 1 for s in shapes]


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def snap(ps):
    return [p.detach().double().cpu().clone() for p in ps]


# ---- the fp64 references (and, in another dtype, the stand-ins) -------------------------------------------------------------------
class TorchSGD:
    """torch.optim.SGD(nesterov) + clip_grad_norm_ on copies of ``init`` in ``dtype``"""

    def __init__(self, init, shapes=SHAPES, dtype=torch.float64, momentum=MOMENTUM, nesterov=True):
        self.ps = [torch.nn.Parameter(t.to(dtype)) for t in init]
        self.opt = torch.optim.SGD(groups_of(self.ps, shapes), lr=LR, momentum=momentum, weight_decay=WD, nesterov=nesterov, foreach=False)

    def step(self, grads, max_norm=MAX_NORM):
        for p, g in zip(self.ps, grads):
            p.grad = None if g is None else g.to(p.dtype).clone()
        live = [p for p in self.ps if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False) if max_norm else None
        self.opt.step()
        return norm

    def state(self, i, key="momentum_buffer"):
        return self.opt.state[self.ps[i]].get(key) if self.ps[i] in self.opt.state else None


class TorchLAMB:
    """optim.lamb_update_torch on copies of ``init`` in ``dtype``"""

    def __init__(self, init, shapes, dtype=torch.float64, max_grad_norm=MAX_GRAD_NORM, use_nvlamb=False, lr=LR):
        self.ps = [t.to(dtype).clone() for t in init]
        self.m = [torch.zeros_like(p) for p in self.ps]
        self.v = [torch.zeros_like(p) for p in self.ps]
        self.group_of = group_index(shapes)
        self.groups = [dict(lr=lr, betas=BETAS, eps=LAMB_EPS, weight_decay=WD), dict(lr=lr, betas=BETAS, eps=LAMB_EPS, weight_decay=0.0)]
        self.st, self.mgn, self.nv, self.seen = {"step": 0}, max_grad_norm, use_nvlamb, [False] * len(init)
        self.last = None

    def step(self, grads, max_norm=MAX_NORM, scale=1.0):
        from mtlora_amd.optim import lamb_update_torch
        gs = [None if g is None else g.to(self.ps[0].dtype) for g in grads]
        self.last = lamb_update_torch(self.ps, gs, self.m, self.v, self.group_of, self.groups, self.st, max_norm, scale, self.mgn, self.nv)
        if not self.last["skipped"]:
            self.seen = [a or g is not None for a, g in zip(self.seen, grads)]
        return self.last["norm"]

    def state(self, i, key):
        return ({"exp_avg": self.m, "exp_avg_sq": self.v}[key][i]) if self.seen[i] else None


# ---- the error measures (test_gpu_optim.py's forms) ---------------------------------------------------------------------------------
def delta_figure(before, after, ref_before, ref_after):
    """per tensor: err = max|delta - delta_ref| and what a relative bound has to cover once the ulp of storing p in fp32 is taken
    off, (err - ulp32(max|p|)) / max|delta_ref|.  Returns (worst such ratio, [(err, max|delta_ref|, ulp)])"""
    rows, worst = [], 0.0
    for b, a, rb, ra in zip(before, after, ref_before, ref_after):
        d, dr = a - b, ra - rb
        err, scale = (d - dr).abs().max().item(), dr.abs().max().item()
        ulp = ulp32(max(a.abs().max().item(), b.abs().max().item()))
        rows.append((err, scale, ulp))
        if scale > 0:
            worst = max(worst, (err - ulp) / scale)
    return worst, rows


def check_delta(what, before, after, ref_before, ref_after, rtol, names=None):
    worst, rows = delta_figure(before, after, ref_before, ref_after)
    fig(f"{what}: max (|delta - delta_ref| - ulp32(max|p|)) / max|delta_ref|", worst)
    for i, (err, scale, ulp) in enumerate(rows):
        assert err <= rtol * scale + ulp, (what, names[i] if names else i, err, rtol * scale + ulp, scale)


def state_figure(got, ref):
    return (got.double().cpu() - ref.double()).abs().max().item() / ref.double().abs().max().item()


def norm_figure(got, ref):
    return abs(float(got) - float(ref)) / float(ref)


# =====================================================================================================================================
def test_sgd_update_torch_is_torch_sgd_in_fp64():
    """sgd_update_torch in fp64 against torch.optim.SGD(nesterov=True, foreach=False) + clip_grad_norm_ over three steps (clip idle,
    idle, active), also with momentum 0 and with nesterov=False: equal to fp64 rounding (a few ulps of the largest value)"""
    from mtlora_amd.optim import sgd_update_torch
    init, grads = common_inputs()
    eps = float(np.finfo(np.float64).eps)
    for mu, nesterov in ((MOMENTUM, True), (0.0, False), (MOMENTUM, False)):
        ref = TorchSGD(init, momentum=mu, nesterov=nesterov)
        ps = [t.double().clone() for t in init]
        bufs = [torch.zeros_like(p) for p in ps]
        groups = [dict(lr=LR, momentum=mu, weight_decay=WD, nesterov=nesterov), dict(lr=LR, momentum=mu, weight_decay=0.0, nesterov=nesterov)]
        for k, gs in enumerate(grads):
            rnorm = ref.step(gs)
            norm, skipped = sgd_update_torch(ps, [g.double() for g in gs], bufs, group_index(), groups, MAX_NORM)
            assert not skipped and norm_figure(norm, rnorm) <= 4 * eps
            assert (rnorm.item() > MAX_NORM) == (k == 2)
            for i, (p, rp) in enumerate(zip(ps, ref.ps)):
                assert (p - rp.detach()).abs().max().item() <= 8 * eps * rp.detach().abs().max().item(), (mu, nesterov, k, i)
                if mu:
                    rb = ref.state(i)
                    assert (bufs[i] - rb).abs().max().item() <= 8 * eps * rb.abs().max().item(), (mu, nesterov, k, i)
                else:
                    assert ref.state(i) is None and not bufs[i].any()  # no momentum: the buffer is not touched
    # unscale and skip: gradients stored at 1024 x give the same step; one inf skips it and nothing is written
    a = [t.double().clone() for t in init]
    b = [t.double().clone() for t in init]
    ba, bb = [torch.zeros_like(p) for p in a], [torch.zeros_like(p) for p in b]
    sgd_update_torch(a, [g.double() for g in grads[1]], ba, group_index(), groups, MAX_NORM)
    sgd_update_torch(b, [g.double() * 1024.0 for g in grads[1]], bb, group_index(), groups, MAX_NORM, scale=1024.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))  # (1024 is a power of two: the unscale is exact)
    bad = [g.double().clone() for g in grads[1]]
    bad[5][7] = float("inf")
    keep = [x.clone() for x in a]
    norm, skipped = sgd_update_torch(a, bad, ba, group_index(), groups, MAX_NORM)
    assert skipped and not torch.isfinite(norm) and all(torch.equal(x, y) for x, y in zip(a, keep))


def test_lamb_update_torch_defining_properties():
    """wd = 0 without nvlamb is bias-corrected Adam; a zero parameter or a zero u gets ratio = lr; a decayed tensor moves by
    lr |p|; max_grad_norm is idle below the threshold and divides by exactly n / max_grad_norm above it"""
    shapes = SHAPES + [ZERO_SHAPE]
    init, grads = common_inputs(shapes, zero=(ZERO_SHAPE,))
    Z = len(shapes) - 1
    ref = TorchLAMB(init, shapes, max_grad_norm=None)
    adam = [torch.nn.Parameter(t.double()) for t in init]
    aopt = torch.optim.Adam(adam, lr=LR, betas=BETAS, eps=LAMB_EPS, foreach=False)  # eps is added to sqrt(v / bc2), as LAMB's
    eps64 = float(np.finfo(np.float64).eps)
    for k, gs in enumerate(grads):
        before = [p.clone() for p in ref.ps]
        ref.step(gs)
        for p, g in zip(adam, gs):
            p.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_(adam, MAX_NORM, foreach=False)
        aopt.step()
        assert ref.st["step"] == k + 1
        for i, s in enumerate(shapes):
            d = ref.ps[i] - before[i]
            if not decays(s):  # wd = 0, use_nvlamb False: ratio = lr, u = Adam's -- the parameters follow torch Adam step for step
                assert ref.last["ratio"][i].item() == LR
                assert (ref.ps[i] - adam[i].detach()).abs().max().item() <= 64 * eps64 * max(1.0, adam[i].detach().abs().max().item()), (k, i)
            elif i == Z and k == 0:  # |p| = 0: ratio = lr although the group decays
                assert ref.last["ratio"][i].item() == LR
            else:  # |delta p| = ratio |u| = lr |p|
                assert abs(d.norm().item() - LR * before[i].norm().item()) <= 1e-12 * LR * before[i].norm().item(), (k, i)
    # a zero u: zero gradient, zero moments, wd = 0 ... and with wd != 0 a zero p as well
    p, m, v = [torch.zeros(8, dtype=torch.float64)], [torch.zeros(8, dtype=torch.float64)], [torch.zeros(8, dtype=torch.float64)]
    other = [torch.ones(8, dtype=torch.float64)]
    from mtlora_amd.optim import lamb_update_torch
    out = lamb_update_torch(p + other, [torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)], m + [torch.zeros(8, dtype=torch.float64)],
                            v + [torch.zeros(8, dtype=torch.float64)], [0, 0], [dict(lr=LR, betas=BETAS, eps=LAMB_EPS, weight_decay=WD)], {"step": 0})
    assert out["ratio"][0].item() == LR and not p[0].any()
    # use_nvlamb: the trust ratio also where wd = 0
    nv = TorchLAMB(init, shapes, use_nvlamb=True)
    b0 = nv.ps[3].clone()
    nv.step(grads[1])
    assert abs((nv.ps[3] - b0).norm().item() - LR * b0.norm().item()) <= 1e-12 * LR * b0.norm().item()
    # max_grad_norm: n is the norm after the max_norm clip
    for k, gs in enumerate(grads):
        on, off = TorchLAMB(init, shapes), TorchLAMB(init, shapes, max_grad_norm=None)
        n = on.step(gs).item()
        off.step(gs)
        n_clipped = min(n, MAX_NORM * n / (n + 1e-6))
        c = on.last["clip"].item()
        if n_clipped > MAX_GRAD_NORM:
            assert k >= 1 and abs(c - n_clipped / MAX_GRAD_NORM) <= 4 * eps64 * c
            # dividing g by c divides m by c and v by c^2 (first step, zero moments)
            assert (on.m[6] * c - off.m[6]).abs().max().item() <= 8 * eps64 * off.m[6].abs().max().item()
            assert (on.v[6] * c * c - off.v[6]).abs().max().item() <= 8 * eps64 * off.v[6].abs().max().item()
        else:
            assert k == 0 and c == 1.0
            assert all(torch.equal(a, b) for a, b in zip(on.ps, off.ps)) and all(torch.equal(a, b) for a, b in zip(on.m, off.m))
    # a skipped step writes nothing and does not count
    r = TorchLAMB(init, shapes)
    r.step(grads[1])
    keep = [x.clone() for x in r.ps + r.m + r.v]
    bad = [g.clone() for g in grads[1]]
    bad[2][5] = float("nan")
    r.step(bad)
    assert r.last["skipped"] and r.st["step"] == 1 and all(torch.equal(x, y) for x, y in zip(r.ps + r.m + r.v, keep))


def test_fp32_standins_against_fp64():
    """what fp32 arithmetic alone costs on the GPU file's inputs: torch.optim.SGD in fp32 and lamb_update_torch in fp32 against
    the fp64 references, in the GPU file's measures.  The GPU file's bounds are the project's (tests/test_gpu_optim.py) unless a
    figure here exceeds a quarter of one, in which case that bound is 4 x the figure; this test asserts the choice recorded there."""
    import test_gpu_optim_sgd_lamb as G
    worst = {"sgd": {"norm": 0.0, "state": 0.0, "delta": 0.0}, "lamb": {"norm": 0.0, "state": 0.0, "delta": 0.0}}
    init, grads = common_inputs()
    ref, lo = TorchSGD(init), TorchSGD(init, dtype=torch.float32)
    for gs in grads:
        rb, lb = snap(ref.ps), snap(lo.ps)
        rn, ln = ref.step(gs), lo.step(gs)
        w = worst["sgd"]
        w["norm"] = max(w["norm"], norm_figure(ln, rn))
        w["delta"] = max(w["delta"], delta_figure(lb, snap(lo.ps), rb, snap(ref.ps))[0])
        w["state"] = max([w["state"]] + [state_figure(lo.state(i), ref.state(i)) for i in range(len(init))])
    shapes = SHAPES + [ZERO_SHAPE]
    init, grads = common_inputs(shapes, zero=(ZERO_SHAPE,))
    ref, lo = TorchLAMB(init, shapes), TorchLAMB(init, shapes, dtype=torch.float32)
    for gs in grads:
        rb, lb = snap(ref.ps), snap(lo.ps)
        rn, ln = ref.step(gs), lo.step(gs)
        w = worst["lamb"]
        w["norm"] = max(w["norm"], norm_figure(ln, rn))
        w["delta"] = max(w["delta"], delta_figure(lb, snap(lo.ps), rb, snap(ref.ps))[0])
        w["state"] = max([w["state"]] + [state_figure(lo.state(i, k), ref.state(i, k)) for i in range(len(init)) for k in ("exp_avg", "exp_avg_sq")])
    project = {"norm": 1e-5, "state": 1e-5, "delta": 2e-4}
    for alg in ("sgd", "lamb"):
        for q in ("norm", "state", "delta"):
            fig(f"fp32 stand-in, {alg}, {q}", worst[alg][q])
            expect = project[q] if worst[alg][q] <= project[q] / 4 else 4 * worst[alg][q]
            have = G.BOUNDS[alg][q]
            assert have == project[q] if expect == project[q] else abs(have - expect) <= 0.05 * expect, (alg, q, worst[alg][q], have)


def test_constructor_rejections():
    """what the new classes refuse, before anything touches a device (CPU parameters: the last refusal is the missing GPU)"""
    from mtlora_amd.optim import FusedAdamW, FusedLAMB, FusedOptimizer, FusedSGD
    assert issubclass(FusedSGD, FusedOptimizer) and issubclass(FusedLAMB, FusedOptimizer) and issubclass(FusedAdamW, FusedOptimizer)
    ps = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(dampening=0.1), dict(maximize=True), dict(nesterov=True), dict(momentum=-0.1), dict(lr=-1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            FusedSGD(ps, **{"lr": 0.1, **kw})
    with pytest.raises(ValueError):
        FusedSGD([{"params": ps, "dampening": 0.5}], lr=0.1)
    for kw in (dict(bias_correction=False), dict(grad_averaging=False), dict(adam_w_mode=False), dict(amsgrad=True), dict(betas=(0.9, 1.0)),
               dict(eps=-1.0), dict(lr=-1.0), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            FusedLAMB(ps, **kw)
    with pytest.raises(ValueError):
        FusedLAMB([{"params": ps, "adam_w_mode": False}])
    for cls, kw in ((FusedSGD, dict(lr=0.1)), (FusedLAMB, {})):
        with pytest.raises(ValueError, match="Python number"):
            cls(ps, **{**kw, "lr": torch.tensor(0.1)})
        with pytest.raises(TypeError, match="fp32 parameters only"):
            cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], **kw)
        # out of scope: accumulation inside the update and the device-side schedule, TypeError naming the class
        opt = cls.__new__(cls)
        opt._capturable = True
        with pytest.raises(TypeError, match=cls.__name__):
            opt.clip_and_step(5.0, None, accumulation_steps=2)
        with pytest.raises(TypeError, match=cls.__name__):
            opt.attach_schedule(None)
        for word in ("accumulation_steps", "attach_schedule", "GraphedTrainStep"):
            assert word in cls.__doc__  # the docstrings say what is out of scope


def test_build_optimizer_names():
    from mtlora_amd import mtl_harness as H
    m = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.LayerNorm(8))
    opt = H.build_optimizer(m, lr=0.1, name="sgd", momentum=0.8)
    assert type(opt) is torch.optim.SGD and len(opt.param_groups) == 2
    g0, g1 = opt.param_groups
    assert (g0["momentum"], g0["nesterov"], g0["dampening"], g0["weight_decay"], g1["weight_decay"], g0["lr"]) == (0.8, True, 0, 0.05, 0.0, 0.1)
    assert [p.shape for p in g0["params"]] == [m[0].weight.shape] and len(g1["params"]) == 3
    assert H.build_optimizer(m, name="SGD").param_groups[0]["momentum"] == 0.9
    for name in ("lamb", "fused_lamb"):
        with pytest.raises(ValueError, match="apex"):
            H.build_optimizer(m, name=name)
    with pytest.raises(ValueError, match="name"):
        H.build_optimizer(m, name="adagrad")
    for name in ("adamw", "fused_adam"):  # what the default arguments build
        a, b = H.build_optimizer(m, name=name), H.build_optimizer(m)
        assert type(a) is type(b) is torch.optim.AdamW
        strip = lambda gs: [{k: v for k, v in g.items() if k != "params"} for g in gs]
        assert strip(a.param_groups) == strip(b.param_groups)
    for name in ("sgd", "lamb", "adamw"):  # impl="hip" on CPU parameters: the class is chosen, then refuses the missing GPU
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            H.build_optimizer(m, name=name, impl="hip")


def test_new_exports_header_and_bindings_agree():
    """the four new prototypes of the header, parameter for parameter in count and in where the doubles sit, against _lib._SIGS;
    the library exports them under ABI 12; the SGD record is the AdamW record's size"""
    import ctypes
    from mtlora_amd import _lib
    raw = open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    ctype_of = {"float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in ("mtlora_sgd_update", "mtlora_sgd_update_dev", "mtlora_lamb_update", "mtlora_lamb_update_dev"):
        assert name in protos and name in _lib._SIGS and name in _lib.EXPORTS, name
        params = [p.strip() for p in protos[name].split(",")]
        res, argtypes = _lib._SIGS[name]
        assert res is ctypes.c_int and len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, p)
            else:
                assert a is ctype_of[p.split()[0]], (name, p, a)
    assert "#define MTLORA_ABI_VERSION 12" in raw and _lib.ABI_VERSION == 12
    assert f"#define MTLORA_LAMB_CTRL_CLIP {_lib.LAMB_CTRL_CLIP}" in raw
    assert ctypes.sizeof(_lib.SgdGroup) == ctypes.sizeof(_lib.AdamwGroup) == 40
    assert [n for n, _ in _lib.SgdGroup._fields_] == re.search(r"typedef struct mtlora_sgd_group \{\s*double ([^;]*);", hdr).group(1).replace(" ", "").split(",")
    L = _lib.lib()
    g = (_lib.SgdGroup * 1)()
    a = (_lib.AdamwGroup * 1)()
    # rejected on the host before any launch: null pointers, too many groups, scratch too small (LAMB needs four words per chunk)
    assert L.mtlora_sgd_update(None, None, 1, 1, g, 1, 0.0, None, None, None, None, 2.0, 0.5, 1, None, 0, None) == -4
    assert L.mtlora_sgd_update(16, 16, 1, 1, g, 17, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 8, None) == -7
    assert L.mtlora_sgd_update(16, 16, 1, 1, g, 1, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 4, None) == -5
    assert L.mtlora_lamb_update(16, 16, 1, 1, a, 1, 0.0, 1.0, 0, 16, None, None, None, 2.0, 0.5, 1, 16, 8, None) == -5
    g[0].momentum = -1.0  # a record the by-value entry rejects
    assert L.mtlora_sgd_update(16, 16, 1, 1, g, 1, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 8, None) == -2
    a[0].beta1 = 1.0
    assert L.mtlora_lamb_update(16, 16, 1, 1, a, 1, 0.0, 1.0, 0, 16, None, None, None, 2.0, 0.5, 1, 16, 16, None) == -2
    assert L.mtlora_sgd_update_dev(16, 16, 1, 1, 12, 1, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 8, None) == -3  # misaligned records
