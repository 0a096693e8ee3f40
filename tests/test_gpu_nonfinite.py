"""Non-finite values: propagation and containment in every autograd node ("Non-finite values").

Each node runs on the same seeded inputs clean and with ONE element of one input (an activation or an incoming gradient) replaced
by NaN or +inf.  The fp64 reference the suite already uses for the node (oracle.mtlora_oracle, F.layer_norm, F.batch_norm + relu,
F.interpolate) is evaluated on the poisoned, dtype-rounded inputs; ``~isfinite(reference)`` is the dependency set.  For every output
and every gradient of the kernel:
  * ``~isfinite(kernel)`` equals that set element for element (nothing swallowed, nothing leaked), and
  * wherever the reference itself is unchanged by the injection the poisoned run is BIT-equal to the clean run (reductions are
    fixed-order: independent elements do not move).
Then fp16 overflow without injection (inf exactly where the fp64 result rounded to fp16 is inf: no saturation, no NaN) and one
end-to-end step whose loss scale overflows the backward: GradScaler and LossScaler + FusedAdamW skip it.

The case classes build inputs and references on the CPU (tests/test_cpu_nonfinite.py checks every reference mask there: not vacuous,
and local where the node is row-, window- or column-local); only ``Case.run`` touches the GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import mtlora_oracle as O

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
F16_MAX = 65504.0


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _rnd(shape, gen, dtype, std=1.0, mean=0.0):
    """seeded N(mean, std) values rounded to ``dtype`` (kept in that dtype): generic and, for all practical purposes, non-zero"""
    return (torch.randn(*shape, generator=gen) * std + mean).to(dtype)


class Poison:
    """one injected element: ``inputs[name][idx] = value``; ``local``: the outputs that stay local for this injection (their reference
    mask must cover less than half of the tensor); ``dead``: the reference says NOTHING depends on the element (a ReLU select)"""

    def __init__(self, name, idx, local=(), dead=False, value=None):
        self.name, self.idx, self.local, self.dead, self.value = name, tuple(idx), tuple(local), dead, value

    def __repr__(self):
        return f"{self.name}{list(self.idx)}"


class Case:
    """a node at one shape: ``inputs()`` (CPU tensors in their storage dtype, built once), ``poisons()``, ``reference(inputs)`` (fp64,
    CPU: every output and gradient by name) and ``run(inputs)`` (the HIP path, same names)"""
    key = ""

    def inputs(self):
        if not hasattr(self, "_inputs"):
            self._inputs = self.make_inputs(torch.Generator().manual_seed(1234))
        return self._inputs

    def poisoned(self, p, value):
        inp = dict(self.inputs())
        t = inp[p.name].clone()
        t[p.idx] = value if p.value is None else p.value
        inp[p.name] = t
        return inp

    def _sets(self, p, value):
        cache = self.__dict__.setdefault("_masks", {})
        k = (repr(p), repr(value if p.value is None else p.value))
        if k not in cache:
            if not hasattr(self, "_clean_ref"):
                self._clean_ref = self.reference(self.inputs())
            ref = self.reference(self.poisoned(p, value))
            cache[k] = ({n: ~torch.isfinite(v) for n, v in ref.items()}, {n: v != self._clean_ref[n] for n, v in ref.items()})
        return cache[k]

    def masks(self, p, value):
        """the dependency sets {output name: bool tensor} of the fp64 reference, cached per (poison, value)"""
        return self._sets(p, value)[0]

    def moved(self, p, value):
        """{output name: where the fp64 reference itself differs from its clean value}: the non-finite set, and the elements an
        infinity reaches as a FINITE change (a key whose score became -inf drops out of the softmax; a NaN under the ReLU's select
        passes the gradient into dbeta).  Everywhere else the reference is bit-unchanged, and so must the kernel be."""
        return self._sets(p, value)[1]


def _d(t, grad=True):
    return t.detach().double().cpu().requires_grad_(grad)


def guard_masks(case, p, masks):
    """the reference alone: the case is not vacuous, and local outputs are local"""
    if p.dead:
        assert not any(bool(m.any()) for m in masks.values()), (case.key, p, "the reference depends on a dead element")
        return
    assert any(bool(m.any()) for m in masks.values()), (case.key, p, "nothing depends on the poisoned element")
    for n in p.local:
        assert n in masks, (case.key, p, n)
        frac = masks[n].float().mean().item()
        assert frac < 0.5, (case.key, p, n, f"reference set covers {frac:.2f} of a local output")


def check_contract(case, value):
    """clean run, then one poisoned run per injection: sets equal to the reference's, bit-equal elsewhere.  Every deviation of the case
    is collected and reported together."""
    clean = {n: v.detach().cpu() for n, v in case.run(case.inputs()).items()}
    bad = []
    for n, v in clean.items():
        if not torch.isfinite(v.float()).all():
            bad.append(f"clean run: {n} is not finite")
    for p in case.poisons():
        masks = case.masks(p, value)
        guard_masks(case, p, masks)
        got = {n: v.detach().cpu() for n, v in case.run(case.poisoned(p, value)).items()}
        assert got.keys() == masks.keys() == clean.keys(), (case.key, sorted(got), sorted(masks))
        for n, exp in masks.items():
            g, c = got[n], clean[n]
            assert g.shape == exp.shape, (case.key, n, g.shape, exp.shape)
            nonfin = ~torch.isfinite(g.float())
            swallowed, leaked = int((exp & ~nonfin).sum()), int((nonfin & ~exp).sum())
            if swallowed or leaked:
                bad.append(f"{p} -> {n}: {swallowed} of {int(exp.sum())} swallowed (finite where the reference is not), "
                           f"{leaked} leaked (non-finite where the reference is finite)")
            keep = ~case.moved(p, value)[n] & ~nonfin
            if not torch.equal(g[keep], c[keep]):
                moved = int((g[keep] != c[keep]).sum())
                bad.append(f"{p} -> {n}: {moved} independent elements are not bit-equal to the clean run")
    assert not bad, f"{case.key} ({value}):\n  " + "\n  ".join(bad)


def _rows(M):
    """first row, last row and the rows either side of a 64-row tile edge"""
    return sorted({0, M - 1} | ({63, 64} if M > 64 else set()))


# ------------------------------------------------------------------------------------------------
# MTLoRALinear: full fine-tuning (dW), BIAS "all" (db) and trainable scales all on
# ------------------------------------------------------------------------------------------------
class LinearCase(Case):
    def __init__(self, dtype, shape):
        self.dtype, self.shape = dtype, shape
        self.key = f"linear{shape}-{dtype}"

    def _module(self):
        from mtlora_amd.lora import MTLoRALinear
        M, K, N, rs, rt, T, use_xt = self.shape
        tasks = [f"t{i}" for i in range(T)] or None
        r = {"shared": rs, **{t: rt for t in (tasks or [])}}
        return MTLoRALinear(K, N, r=r, lora_shared_scale=4.0, lora_task_scale={t: 4.0 for t in tasks} if tasks else 1.0, lora_dropout=0.0,
                            tasks=tasks, trainable_scale_shared=True, trainable_scale_per_task=bool(tasks)), tasks

    def make_inputs(self, gen):
        M, K, N, rs, rt, T, use_xt = self.shape
        m, tasks = self._module()
        self.params = {}
        for n, p in m.named_parameters():
            if "scale" in n:
                self.params[n] = p.detach().clone()
            else:
                self.params[n] = _rnd(p.shape, gen, self.dtype, 0.05 if "lora" in n else 0.02).float()
        inp = {"x": _rnd((M, K), gen, self.dtype), "gy": _rnd((M, N), gen, self.dtype)}
        for i in range(T):
            if use_xt:
                inp[f"x_t{i}"] = _rnd((M, K), gen, self.dtype)
            inp[f"gy_t{i}"] = _rnd((M, N), gen, self.dtype)
        return inp

    def poisons(self):
        M, K, N, rs, rt, T, use_xt = self.shape
        ps = []
        for i, m in enumerate(_rows(M)):
            k, n = ((0, 0) if i % 2 == 0 else (K - 1, N - 1))
            ps.append(Poison("x", (m, k), local=["y", "linear.weight"]))
            ps.append(Poison("gy", (m, n), local=["dx", "linear.weight", "linear.bias", "lora_shared_B"]))
        if T:
            if use_xt:
                ps.append(Poison("x_t1", (M - 1, 3), local=["y", "y_t0", "y_t1", "dx", "linear.weight"]))
            ps.append(Poison("gy_t1", (64, N - 2), local=["dx", "linear.weight", "linear.bias", "lora_tasks_B.t1"] + (["dx_t1"] if use_xt else [])))
        return ps

    def reference(self, inp):
        M, K, N, rs, rt, T, use_xt = self.shape
        tasks = [f"t{i}" for i in range(T)] or None
        P = {n: _d(v) for n, v in self.params.items()}
        x = _d(inp["x"])
        xt = {t: _d(inp[f"x_t{i}"]) for i, t in enumerate(tasks)} if (tasks and use_xt) else None
        y, yt = O.mtlora_linear(x, P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], P["lora_shared_scale"],
                                tasks=tasks, A_t={t: P["lora_tasks_A." + t] for t in tasks} if tasks else None,
                                B_t={t: P["lora_tasks_B." + t] for t in tasks} if tasks else None,
                                scale_t={t: P["lora_task_scale." + t] for t in tasks} if tasks else None, x_tasks=xt)
        outs = [y] + [yt[t] for t in (tasks or [])]
        torch.autograd.backward(outs, [inp["gy"].double()] + [inp[f"gy_t{i}"].double() for i in range(T)])
        res = {"y": y.detach(), "dx": x.grad}
        for i, t in enumerate(tasks or []):
            res[f"y_t{i}"] = yt[t].detach()
            if use_xt:
                res[f"dx_t{i}"] = xt[t].grad
        res.update({n: p.grad for n, p in P.items()})
        return res

    def run(self, inp):
        M, K, N, rs, rt, T, use_xt = self.shape
        m, tasks = self._module()
        m.load_state_dict(self.params)
        m = m.to(dev())
        x = inp["x"].to(dev()).requires_grad_(True)
        xt = {t: inp[f"x_t{i}"].to(dev()).requires_grad_(True) for i, t in enumerate(tasks)} if (tasks and use_xt) else None
        y, yt = m(x, xt)
        outs = [y] + [yt[t] for t in (tasks or [])]
        torch.autograd.backward(outs, [inp["gy"].to(dev())] + [inp[f"gy_t{i}"].to(dev()) for i in range(T)])
        res = {"y": y, "dx": x.grad}
        for i, t in enumerate(tasks or []):
            res[f"y_t{i}"] = yt[t]
            if use_xt:
                res[f"dx_t{i}"] = xt[t].grad
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            res[n] = p.grad
        return res


# the smallest off-grid geometry of test_linear_random_vs_oracle whose task outputs read their own x_t, and its smallest T = 0 one
LINEAR_SHAPES = [(520, 384, 96, 64, 4, 4, True), (1000, 96, 288, 64, 4, 0, False)]
LINEAR_CASES = {(dt, s): LinearCase(dt, s) for dt in (F16, BF16) for s in LINEAR_SHAPES}


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=["t4", "t0"])
def test_linear_nonfinite(shape, dtype, value):
    """(t4 is what found the shared-accumulator leak of the wave-streaming Q pass, DESIGN.md 8g: a NaN in gy_t1 row 64 used to reach
    row 64 of dx_t0 / t2 / t3 and all of lora_tasks_A.t0 / t2 / t3 in every family but [tiled])"""
    check_contract(LINEAR_CASES[dtype, shape], value)


# ------------------------------------------------------------------------------------------------
# task-enabled Mlp: MlpHidFn (implicit task hiddens) and the per-layer path (fc1 with the GELU written by its epilogue, fc2 with
# gelu' in its dX epilogue); geometry c2s0 of test_mlp_implicit_task_hiddens
# ------------------------------------------------------------------------------------------------
def _fp64_linear(P, pre, s_s, s_t, tasks, x, xt):
    base = x @ P[f"{pre}.linear.weight"].t() + P[f"{pre}.linear.bias"]
    ys = base + s_s * (x @ P[f"{pre}.lora_shared_A"].t()) @ P[f"{pre}.lora_shared_B"].t()
    return ys, [base + s_t[t] * (xt[i] @ P[f"{pre}.lora_tasks_A.{t}"].t()) @ P[f"{pre}.lora_tasks_B.{t}"].t() for i, t in enumerate(tasks)]


class MlpCase(Case):
    C, Hd, T, r_t, M = 96, 384, 4, 4, 3 * 977

    def __init__(self, dtype, hid):
        self.dtype, self.hid = dtype, hid
        self.tasks = [f"t{i}" for i in range(self.T)]
        self.key = f"mlp-{'hid' if hid else 'layers'}-{dtype}"

    def _module(self):
        from mtlora_amd import mtl_harness as H
        from mtlora_amd.swin_transformer_mtlora import Mlp
        ns = H.mtlora_namespace(self.tasks, r_shared=16, r_task=self.r_t, scale=2.0, dropout=0.0)
        return Mlp(self.C, self.Hd, lora=True, tasks=self.tasks, mtlora=ns, layer_idx=0)

    def make_inputs(self, gen):
        mlp = self._module()
        self.params = {n: _rnd(p.shape, gen, self.dtype, 0.1 if "lora_" in n else 0.05).float() for n, p in mlp.named_parameters()}
        self.scales = {pre: (float(getattr(mlp, pre).lora_shared_scale), {t: float(getattr(mlp, pre).lora_task_scale[t]) for t in self.tasks})
                       for pre in ("fc1", "fc2")}
        inp = {}
        for i in range(1 + self.T):
            inp[f"x{i}"] = _rnd((self.M, self.C), gen, self.dtype).float()  # (fp32 streams under autocast, values on the 16-bit grid)
            inp[f"g{i}"] = _rnd((self.M, self.C), gen, self.dtype)
        return inp

    def poisons(self):
        M, C = self.M, self.C
        ps = []
        for i, m in enumerate(_rows(M)):
            c = 0 if i % 2 == 0 else C - 1
            ps.append(Poison("x0", (m, c), local=["y0"]))
            ps.append(Poison("g0", (m, c), local=["dx0"]))
        ps.append(Poison("x2", (64, 5), local=["y0", "y2", "dx0", "dx2"]))
        ps.append(Poison("g2", (M - 1, C - 1), local=["dx0", "dx2"]))
        return ps

    def reference(self, inp):
        P = {n: _d(v, "lora_" in n) for n, v in self.params.items()}
        X = [_d(inp[f"x{i}"]) for i in range(1 + self.T)]
        h, ht = _fp64_linear(P, "fc1", *self.scales["fc1"], self.tasks, X[0], X[1:])
        y, yt = _fp64_linear(P, "fc2", *self.scales["fc2"], self.tasks, F.gelu(h), [F.gelu(v) for v in ht])
        outs = [y] + yt
        torch.autograd.backward(outs, [inp[f"g{i}"].double() for i in range(1 + self.T)])
        res = {f"y{i}": o.detach() for i, o in enumerate(outs)}
        res.update({f"dx{i}": x.grad for i, x in enumerate(X)})
        res.update({n: p.grad for n, p in P.items() if p.requires_grad})
        return res

    def run(self, inp):
        from mtlora_amd import functional as Fn
        mlp = self._module()
        mlp.load_state_dict(self.params)
        mlp = mlp.to(dev()).train()
        for n, p in mlp.named_parameters():
            p.requires_grad_("lora_" in n)
        X = [inp[f"x{i}"].to(dev()).requires_grad_(True) for i in range(1 + self.T)]
        old = Fn.set_mlp_hid(self.hid)
        try:
            with torch.autocast("cuda", dtype=self.dtype):
                y, yt = mlp(X[0], {t: X[1 + i] for i, t in enumerate(self.tasks)})
            outs = [y] + [yt[t] for t in self.tasks]
            torch.autograd.backward(outs, [inp[f"g{i}"].to(dev()) for i in range(1 + self.T)])
        finally:
            Fn.set_mlp_hid(old)
        res = {f"y{i}": o for i, o in enumerate(outs)}
        res.update({f"dx{i}": x.grad for i, x in enumerate(X)})
        res.update({n: p.grad for n, p in mlp.named_parameters() if p.requires_grad})
        return res


class GeluPairCase(Case):
    """fc1 with ``gelu_out`` (pre-activation h and gelu(h) from one epilogue) into fc2 with ``gelu_gate`` (gelu'(h) in the dX epilogue),
    h and gelu(h) returned: an infinite x row makes h = +-inf, where exact GELU gives +inf and NaN (-inf * 0).  ``gate_only``: fc2 alone on
    given pre-activations, one of them poisoned (NaN / +inf and, always, -inf)."""
    C, Hd, M = 96, 384, 3 * 211

    def __init__(self, dtype, gate_only):
        self.dtype, self.gate_only = dtype, gate_only
        self.tasks = ["a", "b"]
        self.key = f"mlp-gelu-{'gate' if gate_only else 'pair'}-{dtype}"

    def _modules(self):
        from mtlora_amd.lora import MTLoRALinear
        r, sc = {"shared": 16, "a": 4, "b": 4}, {"a": 1.0, "b": 0.5}
        mk = lambda K, N: MTLoRALinear(K, N, r=r, lora_shared_scale=2.0, lora_task_scale=sc, lora_dropout=0.0, tasks=self.tasks)
        return {"fc1": mk(self.C, self.Hd), "fc2": mk(self.Hd, self.C)}

    def make_inputs(self, gen):
        self.params = {f"{pre}.{n}": _rnd(p.shape, gen, self.dtype, 0.1 if "lora_" in n else 0.05).float()
                       for pre, m in self._modules().items() for n, p in m.named_parameters()}
        self.scales = {pre: (2.0, {"a": 1.0, "b": 0.5}) for pre in ("fc1", "fc2")}
        W = self.Hd if self.gate_only else self.C
        inp = {}
        for i in range(3):
            inp[f"x{i}"] = _rnd((self.M, W), gen, self.dtype, 1.5)
            inp[f"g{i}"] = _rnd((self.M, self.C), gen, self.dtype)
        return inp

    def poisons(self):
        M, W = self.M, (self.Hd if self.gate_only else self.C)
        loc = ["y0", "dx0"] + ([] if self.gate_only else ["h0", "a0"])
        ps = [Poison("x0", (m, 0 if i % 2 == 0 else W - 1), local=loc) for i, m in enumerate(_rows(M))]
        ps += [Poison("x0", (m, 7), local=loc, value=-INF) for m in (0, M - 1)]
        ps += [Poison("x1", (64, 9), local=["y1", "dx1"]), Poison("x2", (63, 9), local=["y2", "dx2"], value=-INF)]
        ps += [Poison("g0", (M - 1, self.C - 1), local=["dx0"]), Poison("g1", (0, 0), local=["dx1"])]
        return ps

    def reference(self, inp):
        P = {n: _d(v, "lora_" in n) for n, v in self.params.items()}
        X = [_d(inp[f"x{i}"]) for i in range(3)]
        res = {}
        if self.gate_only:
            h, ht = X[0], X[1:]
        else:
            h, ht = _fp64_linear(P, "fc1", *self.scales["fc1"], self.tasks, X[0], X[1:])
        a, at = F.gelu(h), [F.gelu(v) for v in ht]
        y, yt = _fp64_linear(P, "fc2", *self.scales["fc2"], self.tasks, a, at)
        outs = [y] + yt
        torch.autograd.backward(outs, [inp[f"g{i}"].double() for i in range(3)])
        if not self.gate_only:
            res.update({f"h{i}": v.detach() for i, v in enumerate([h] + ht)})
            res.update({f"a{i}": v.detach() for i, v in enumerate([a] + at)})
        res.update({f"y{i}": o.detach() for i, o in enumerate(outs)})
        res.update({f"dx{i}": x.grad for i, x in enumerate(X)})
        res.update({n: p.grad for n, p in P.items() if p.requires_grad and p.grad is not None})
        return res

    def run(self, inp):
        from mtlora_amd import functional as Fn
        mods = self._modules()
        for pre, m in mods.items():
            m.load_state_dict({n[len(pre) + 1:]: v for n, v in self.params.items() if n.startswith(pre + ".")})
            m.to(dev()).train()
            m.linear.weight.requires_grad_(False)
            m.linear.bias.requires_grad_(False)
        fc1, fc2 = mods["fc1"], mods["fc2"]
        X = [inp[f"x{i}"].to(dev()).requires_grad_(True) for i in range(3)]
        td = lambda lst: {t: lst[1 + i] for i, t in enumerate(self.tasks)}
        res = {}
        if self.gate_only:
            a = [Fn.GeluDeferredGradFn.apply(h) for h in X]
            y, yt = fc2(a[0], td(a), gelu_gate=(X[0], td(X)))
        else:
            h, h_t, a, a_t = fc1(X[0], td(X), gelu_out=True)
            y, yt = fc2(a, a_t, gelu_gate=(h.detach(), {t: v.detach() for t, v in h_t.items()}))
            res.update({f"h{i}": v for i, v in enumerate([h] + [h_t[t] for t in self.tasks])})
            res.update({f"a{i}": v for i, v in enumerate([a] + [a_t[t] for t in self.tasks])})
        outs = [y] + [yt[t] for t in self.tasks]
        torch.autograd.backward(outs, [inp[f"g{i}"].to(dev()) for i in range(3)])
        res.update({f"y{i}": o for i, o in enumerate(outs)})
        res.update({f"dx{i}": x.grad for i, x in enumerate(X)})
        for pre, m in mods.items():
            if not (self.gate_only and pre == "fc1"):
                res.update({f"{pre}.{n}": p.grad for n, p in m.named_parameters() if p.requires_grad})
        return res


MLP_CASES = {(dt, k): (MlpCase(dt, k == "hid") if k in ("hid", "layers") else GeluPairCase(dt, k == "gate"))
             for dt in (F16, BF16) for k in ("hid", "layers", "pair", "gate")}


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["hid", "layers", "pair", "gate"])
def test_mlp_nonfinite(kind, dtype, value):
    """(hid and layers found the same leak in k_hid_fwd_d / k_hid_bwd_d and behind the fused-GELU layers; the -inf pre-activations
    keep exact GELU's NaN)"""
    check_contract(MLP_CASES[dtype, kind], value)


# ------------------------------------------------------------------------------------------------
# LayerNorm family
# ------------------------------------------------------------------------------------------------
def _scale_kept(n, B):
    """DropPath factors with every sample kept (1 / keep); a dropped sample is out of scope"""
    return torch.full((n, B), 1.0 / 0.7)


class LayerNormCase(Case):
    """kinds: plain, fork (LayerNormFn), residual / residual_noscale (ResidualLayerNormFn), over (M, C) rows"""

    def __init__(self, kind, M, C, xdt, ydt):
        self.kind, self.M, self.C, self.xdt, self.ydt = kind, M, C, xdt, ydt
        self.key = f"layernorm-{kind}-{M}x{C}-{xdt}-{ydt}"

    def make_inputs(self, gen):
        M, C = self.M, self.C
        inp = {"x": _rnd((1, M, C), gen, self.xdt, 2.0, 0.5), "w": _rnd((C,), gen, F32, 0.2, 1.0), "b": _rnd((C,), gen, F32, 0.1),
               "gy": _rnd((1, M, C), gen, self.ydt)}
        if self.kind != "plain":
            inp["gskip"] = _rnd((1, M, C), gen, self.xdt)
        if self.kind.startswith("residual"):
            inp["branch"] = _rnd((1, M, C), gen, self.ydt)
        return inp

    def poisons(self):
        M, C = self.M, self.C
        res = self.kind.startswith("residual")
        ps = []
        for i, m in enumerate(_rows(M)):
            c = 0 if i % 2 == 0 else C - 1
            ps.append(Poison("x", (0, m, c), local=["y", "dx"] + (["xnew", "dbranch"] if res else [])))
            ps.append(Poison("gy", (0, m, c), local=["dx", "dgamma", "dbeta"] + (["dbranch"] if res else [])))
        if self.kind != "plain":
            ps.append(Poison("gskip", (0, M - 1, 0), local=["dx"] + (["dbranch"] if res else [])))
        if res:
            ps.append(Poison("branch", (0, 0, C - 1), local=["y", "dx", "xnew", "dbranch"]))
        return ps

    def _scale(self):
        return _scale_kept(1, 1)[0] if self.kind == "residual" else None

    def reference(self, inp):
        C = self.C
        x, w, b = _d(inp["x"]), _d(inp["w"]), _d(inp["b"])
        res = {}
        if self.kind.startswith("residual"):
            br = _d(inp["branch"])
            s = 1.0 if self._scale() is None else self._scale().double().view(1, 1, 1)
            xn = x + s * br
            y = F.layer_norm(xn, (C,), w, b, 1e-5)
            torch.autograd.backward([xn, y], [inp["gskip"].double(), inp["gy"].double()])
            res.update(xnew=xn.detach(), dbranch=br.grad)
        else:
            y = F.layer_norm(x, (C,), w, b, 1e-5)
            if self.kind == "fork":
                torch.autograd.backward([x, y], [inp["gskip"].double(), inp["gy"].double()])
            else:
                y.backward(inp["gy"].double())
        res.update(y=y.detach(), dx=x.grad, dgamma=w.grad, dbeta=b.grad)
        return res

    def run(self, inp):
        from mtlora_amd import functional as Fn
        x, w, b = (inp[k].to(dev()).requires_grad_(True) for k in ("x", "w", "b"))
        res = {}
        if self.kind.startswith("residual"):
            br = inp["branch"].to(dev()).requires_grad_(True)
            sc = self._scale()
            xn, y = Fn.ResidualLayerNormFn.apply(x, br, None if sc is None else sc.to(dev()), w, b, 1e-5, self.ydt)
            torch.autograd.backward([xn, y], [inp["gskip"].to(dev()), inp["gy"].to(dev())])
            res.update(xnew=xn, dbranch=br.grad)
        elif self.kind == "fork":
            xs, y = Fn.LayerNormFn.apply(x, w, b, 1e-5, self.ydt, None, True)
            torch.autograd.backward([xs, y], [inp["gskip"].to(dev()), inp["gy"].to(dev())])
        else:
            y = Fn.LayerNormFn.apply(x, w, b, 1e-5, self.ydt)
            y.backward(inp["gy"].to(dev()))
        res.update(y=y, dx=x.grad, dgamma=w.grad, dbeta=b.grad)
        return res


class LayerNormStreamsCase(Case):
    """kinds: multi (ResidualLayerNormMultiFn: one shortcut, n branches), merge (ResidualMergeNormStreamsFn on n streams), merge_res
    (the same with per-stream residual + branch); n = 3 streams, B = 2, H = W = 4, C = 96"""
    n, B, H, W, C = 3, 2, 4, 4, 96

    def __init__(self, kind, xdt, ydt):
        self.kind, self.xdt, self.ydt = kind, xdt, ydt
        self.key = f"layernorm-{kind}-{xdt}-{ydt}"

    def make_inputs(self, gen):
        n, B, L, C = self.n, self.B, self.H * self.W, self.C
        Cn = C if self.kind == "multi" else 4 * C
        inp = {"w": _rnd((Cn,), gen, F32, 0.1, 1.0), "b": _rnd((Cn,), gen, F32, 0.1)}
        if self.kind == "multi":
            inp["sc"] = _rnd((B, L, C), gen, self.xdt)
        for k in range(n):
            if self.kind != "multi":
                inp[f"res{k}"] = _rnd((B, L, C), gen, self.xdt)
            if self.kind != "merge":
                inp[f"br{k}"] = _rnd((B, L, C), gen, self.ydt)
            if self.kind == "multi":
                inp[f"gskip{k}"] = _rnd((B, L, C), gen, self.xdt)
                inp[f"gy{k}"] = _rnd((B, L, C), gen, self.ydt)
        if self.kind != "multi":
            inp["g"] = _rnd((n * B, L // 4, 4 * C), gen, self.ydt)
        return inp

    def poisons(self):
        n, B, L, C = self.n, self.B, self.H * self.W, self.C
        if self.kind == "multi":
            k_loc = lambda k: [f"xnew{k}", f"y{k}", f"dbr{k}", "dsc"]
            return [Poison("sc", (0, 0, 0), local=[f"y{k}" for k in range(n)] + ["dsc"]),
                    Poison("br1", (B - 1, L - 1, C - 1), local=k_loc(1)), Poison("br2", (0, 3, 5), local=k_loc(2)),
                    Poison("gy1", (0, 0, 0), local=["dbr1", "dsc", "dgamma", "dbeta"]),
                    Poison("gy0", (B - 1, L - 1, C - 1), local=["dbr0", "dsc", "dgamma", "dbeta"]),
                    Poison("gskip2", (1, 2, 3), local=["dbr2", "dsc"])]
        src = "res" if self.kind == "merge" else "br"
        loc = lambda k: ["y", f"dres{k}"] + ([f"dbr{k}"] if self.kind == "merge_res" else [])
        ps = [Poison(f"{src}1", (0, 0, 0), local=loc(1)), Poison(f"{src}2", (B - 1, L - 1, C - 1), local=loc(2)),
              Poison("g", (0, 0, 0), local=loc(0) + ["dgamma", "dbeta"]),
              Poison("g", (n * B - 1, L // 4 - 1, 4 * C - 1), local=loc(2) + ["dgamma", "dbeta"]),
              Poison("g", (B, 1, 2 * C + 1), local=loc(1) + ["dgamma", "dbeta"])]
        if self.kind == "merge_res":
            ps.append(Poison("res0", (1, 5, 7), local=loc(0)))
        return ps

    def _gather(self, x):
        B, H, W, C = self.B, self.H, self.W, self.C
        return x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)

    def reference(self, inp):
        n, B = self.n, self.B
        w, b = _d(inp["w"]), _d(inp["b"])
        sc = _scale_kept(n, B).double()
        res = {}
        if self.kind == "multi":
            s = _d(inp["sc"])
            brs = [_d(inp[f"br{k}"]) for k in range(n)]
            xs = [s + sc[k].view(B, 1, 1) * brs[k] for k in range(n)]
            ys = [F.layer_norm(x, (self.C,), w, b, 1e-5) for x in xs]
            torch.autograd.backward(xs + ys, [inp[f"gskip{k}"].double() for k in range(n)] + [inp[f"gy{k}"].double() for k in range(n)])
            for k in range(n):
                res.update({f"xnew{k}": xs[k].detach(), f"y{k}": ys[k].detach(), f"dbr{k}": brs[k].grad})
            res["dsc"] = s.grad
        else:
            rs = [_d(inp[f"res{k}"]) for k in range(n)]
            brs = [_d(inp[f"br{k}"]) for k in range(n)] if self.kind == "merge_res" else None
            xs = rs if brs is None else [rs[k] + sc[k].view(B, 1, 1) * brs[k] for k in range(n)]
            y = torch.cat([F.layer_norm(self._gather(x), (4 * self.C,), w, b, 1e-5) for x in xs], 0)
            y.backward(inp["g"].double())
            res["y"] = y.detach()
            for k in range(n):
                res[f"dres{k}"] = rs[k].grad
                if brs is not None:
                    res[f"dbr{k}"] = brs[k].grad
        res.update(dgamma=w.grad, dbeta=b.grad)
        return res

    def run(self, inp):
        from mtlora_amd import functional as Fn
        n, B = self.n, self.B
        w, b = inp["w"].to(dev()).requires_grad_(True), inp["b"].to(dev()).requires_grad_(True)
        sc = _scale_kept(n, B).to(dev())
        up = lambda name: inp[name].to(dev()).requires_grad_(True)
        res = {}
        if self.kind == "multi":
            s, brs = up("sc"), [up(f"br{k}") for k in range(n)]
            outs = Fn.ResidualLayerNormMultiFn.apply(sc, w, b, 1e-5, self.ydt, n, s, *brs)
            torch.autograd.backward(list(outs), [inp[f"gskip{k}"].to(dev()) for k in range(n)] + [inp[f"gy{k}"].to(dev()) for k in range(n)])
            for k in range(n):
                res.update({f"xnew{k}": outs[k], f"y{k}": outs[n + k], f"dbr{k}": brs[k].grad})
            res["dsc"] = s.grad
        else:
            rs = [up(f"res{k}") for k in range(n)]
            brs = [up(f"br{k}") for k in range(n)] if self.kind == "merge_res" else []
            y = Fn.ResidualMergeNormStreamsFn.apply(sc if brs else None, w, b, 1e-5, self.ydt, self.H, self.W, n, *rs, *brs)
            y.backward(inp["g"].to(dev()))
            res["y"] = y
            for k in range(n):
                res[f"dres{k}"] = rs[k].grad
                if brs:
                    res[f"dbr{k}"] = brs[k].grad
        res.update(dgamma=w.grad, dbeta=b.grad)
        return res


LN_DTYPES = [(F32, BF16), (F16, F16)]
LN_CASES = {}
for _xdt, _ydt in LN_DTYPES:
    for _M, _C in [(65, 96), (3, 2048), (50, 40)]:
        for _kind in ("plain", "fork", "residual", "residual_noscale"):
            LN_CASES[_kind, f"{_M}x{_C}", _ydt] = LayerNormCase(_kind, _M, _C, _xdt, _ydt)
    for _kind in ("multi", "merge", "merge_res"):
        LN_CASES[_kind, "streams", _ydt] = LayerNormStreamsCase(_kind, _xdt, _ydt)


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", list(LN_CASES), ids=lambda k: f"{k[0]}-{k[1]}-{str(k[2])[6:]}")
def test_layernorm_family_nonfinite(case, value):
    check_contract(LN_CASES[case], value)


# ------------------------------------------------------------------------------------------------
# BatchNorm (+ ReLU)
# ------------------------------------------------------------------------------------------------
class BatchNormCase(Case):
    def __init__(self, R, C, relu, dtype):
        self.R, self.C, self.relu, self.dtype = R, C, relu, dtype
        self.key = f"batchnorm-{R}x{C}-relu{int(relu)}-{dtype}"

    def make_inputs(self, gen):
        R, C = self.R, self.C
        return {"x": _rnd((R, C), gen, self.dtype, 1.5, 0.3), "w": _rnd((C,), gen, F32, 0.2, 1.0), "b": _rnd((C,), gen, F32, 0.3),
                "g": _rnd((R, C), gen, self.dtype)}

    def _clean_y(self):
        if not hasattr(self, "_y"):
            self._y = self.reference(self.inputs())["y"]
        return self._y

    def _col(self, r, positive, order):
        """a column of row r whose clean output is clearly positive / clearly clipped by the ReLU, scanning in ``order``"""
        y = self._clean_y()[r]
        for c in order:
            if (y[c] > 0.1) if positive else (y[c] == 0):
                return c
        raise AssertionError((self.key, r, positive))

    def poisons(self):
        R, C = self.R, self.C
        ps = []
        col = ["y", "dx", "running_mean", "running_var", "dgamma", "dbeta"]
        for i, r in enumerate(_rows(R)):
            order = range(C) if i % 2 == 0 else range(C - 1, -1, -1)
            ps.append(Poison("x", (r, 0 if i % 2 == 0 else C - 1), local=col))
            # (under the ReLU a gradient only counts where the output is positive: the generic positions take such a column)
            ps.append(Poison("g", (r, self._col(r, True, order) if self.relu else order[0]), local=col))
        if self.relu:  # the select of threshold_backward: a gradient at a clipped position reaches nothing at all
            ps.append(Poison("g", (R // 2, self._col(R // 2, False, range(C))), dead=True))
            ps.append(Poison("g", (R // 2, self._col(R // 2, True, range(C))), local=col))
        return ps

    def reference(self, inp):
        C = self.C
        x, w, b = _d(inp["x"]), _d(inp["w"]), _d(inp["b"])
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
        y = F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
        if self.relu:
            y = torch.relu(y)
        y.backward(inp["g"].double())
        return dict(y=y.detach(), running_mean=rm, running_var=rv, dx=x.grad, dgamma=w.grad, dbeta=b.grad)

    def run(self, inp):
        from mtlora_amd import functional as Fn
        x, w, b = (inp[k].to(dev()).requires_grad_(True) for k in ("x", "w", "b"))
        rm, rv = torch.zeros(self.C, device=dev()), torch.ones(self.C, device=dev())
        y = Fn.BatchNormReluFn.apply(x, w, b, rm, rv, 0.1, 1e-5, self.relu)
        y.backward(inp["g"].to(dev()))
        return dict(y=y, running_mean=rm, running_var=rv, dx=x.grad, dgamma=w.grad, dbeta=b.grad)


BN_CASES = {(R, C, relu, dt): BatchNormCase(R, C, relu, dt) for R, C in [(100, 8), (777, 64)] for relu in (True, False) for dt in (F16, BF16)}


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", list(BN_CASES), ids=lambda k: f"{k[0]}x{k[1]}-relu{int(k[2])}-{str(k[3])[6:]}")
def test_batchnorm_relu_nonfinite(case, value):
    check_contract(BN_CASES[case], value)


# ------------------------------------------------------------------------------------------------
# window attention
# ------------------------------------------------------------------------------------------------
class AttentionCase(Case):
    """mask forms: ids (region ids), densemask, none (shift 0)"""

    def __init__(self, cfg, mask_form, dtype):
        self.cfg, self.mask_form, self.dtype = cfg, mask_form, dtype
        self.key = f"attention-{cfg}-{mask_form}-{dtype}"

    def make_inputs(self, gen):
        B, H, W, nH, ws, shift = self.cfg
        C, N = nH * 32, ws * ws
        return {"qkv": _rnd((B, H, W, 3 * C), gen, self.dtype, 0.7), "bias": _rnd((nH, N, N), gen, F32, 0.5),
                "g": _rnd((B, H, W, C), gen, self.dtype)}

    def poisons(self):
        B, H, W, nH, ws, shift = self.cfg
        C = nH * 32
        h = nH - 1 if nH > 1 else 0
        ps = []
        loc = ["out", "dqkv", "dbias"]
        # one token inside the first image, one in the last window of the last image (the persistent loops' final iteration)
        for (b, i, j), hh in (((0, 3, 4), h), ((B - 1, H - 1, W - 1), 0)):
            for which in range(3):
                # (a key or value reaches every score of its window: that head's whole dbias, which sums over the windows)
                ps.append(Poison("qkv", (b, i, j, which * C + hh * 32 + 5 + which), local=loc if which == 0 else loc[:2]))
            ps.append(Poison("g", (b, i, j, hh * 32 + 31), local=loc))
        return ps

    def _mask(self):
        B, H, W, nH, ws, shift = self.cfg
        return O.shifted_window_mask(H, W, ws, shift)

    def reference(self, inp):
        B, H, W, nH, ws, shift = self.cfg
        C, N = nH * 32, ws * ws
        q, bias = _d(inp["qkv"]), _d(inp["bias"])
        mask = self._mask()
        win = O.roll_and_window_partition(q, shift, ws).reshape(-1, N, 3 * C)
        core = O.window_attention_core(win, bias, None if mask is None else mask.double(), nH, 32 ** -0.5)
        out = O.window_merge_and_roll(core.reshape(-1, ws, ws, C), shift, ws, H, W)
        out.backward(inp["g"].double())
        return dict(out=out.detach(), dqkv=q.grad, dbias=bias.grad)

    def run(self, inp):
        from mtlora_amd import functional as Fn
        from mtlora_amd.swin_transformer_mtlora import _shift_regions
        B, H, W, nH, ws, shift = self.cfg
        q, bias = inp["qkv"].to(dev()).requires_grad_(True), inp["bias"].to(dev()).requires_grad_(True)
        meta = Fn.AttnMeta(B=B, H=H, W=W, window_size=ws, shift=shift, num_heads=nH, head_dim=32, image_layout=True, scale=32 ** -0.5)
        mask = ids = None
        if self.mask_form == "ids":
            ids = _shift_regions(H, W, ws, shift).to(torch.int32).to(dev())
        elif self.mask_form == "densemask":
            mask = self._mask().to(dev())
        out = Fn.WindowAttentionFn.apply(meta, q, bias, mask, ids)
        out.backward(inp["g"].to(dev()))
        return dict(out=out, dqkv=q.grad, dbias=bias.grad)


# (B, H, W, heads, ws, shift): two cases of test_attention_core_vs_oracle and the smallest window-12 case of test_gpu_attention_wide
ATTN_GEOMS = [((2, 14, 14, 3, 7, 3), "ids"), ((2, 14, 14, 3, 7, 3), "densemask"), ((1, 14, 21, 2, 7, 0), "none"), ((3, 12, 12, 6, 12, 0), "none")]
ATTN_CASES = {(g, f, dt): AttentionCase(g, f, dt) for g, f in ATTN_GEOMS for dt in (F16, BF16)}


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", list(ATTN_CASES), ids=lambda k: f"{'x'.join(map(str, k[0]))}-{k[1]}-{str(k[2])[6:]}")
def test_window_attention_nonfinite(case, value):
    check_contract(ATTN_CASES[case], value)


# ------------------------------------------------------------------------------------------------
# residual + DropPath (every sample kept) and the heads' concat + upsample
# ------------------------------------------------------------------------------------------------
class DropPathCase(Case):
    n, B, L, C = 3, 6, 49, 96

    def __init__(self, shared, rdt, ydt):
        self.shared, self.rdt, self.ydt = shared, rdt, ydt
        self.key = f"droppath-shared{int(shared)}-{rdt}-{ydt}"

    def make_inputs(self, gen):
        shp = (self.B, self.L, self.C)
        inp = {f"res{k}": _rnd(shp, gen, self.rdt) for k in range(1 if self.shared else self.n)}
        for k in range(self.n):
            inp[f"y{k}"] = _rnd(shp, gen, self.ydt)
            inp[f"g{k}"] = _rnd(shp, gen, self.rdt)
        return inp

    def poisons(self):
        B, L, C = self.B, self.L, self.C
        every = [f"out{k}" for k in range(self.n)] + [f"dy{k}" for k in range(self.n)] + [f"dres{k}" for k in range(1 if self.shared else self.n)]
        return [Poison("res0", (0, 0, 0), local=every), Poison("y1", (B - 1, L - 1, C - 1), local=every),
                Poison("g2", (2, 7, 9), local=every), Poison("g0", (B - 1, L - 1, C - 1), local=every)]

    def reference(self, inp):
        n, B = self.n, self.B
        sc = _scale_kept(n, B).double()
        res = [_d(inp[f"res{k}"]) for k in range(1 if self.shared else n)]
        ys = [_d(inp[f"y{k}"]) for k in range(n)]
        outs = [(res[0] if self.shared else res[k]) + sc[k].view(B, 1, 1) * ys[k] for k in range(n)]
        torch.autograd.backward(outs, [inp[f"g{k}"].double() for k in range(n)])
        r = {f"out{k}": outs[k].detach() for k in range(n)}
        r.update({f"dy{k}": ys[k].grad for k in range(n)})
        r.update({f"dres{k}": t.grad for k, t in enumerate(res)})
        return r

    def run(self, inp):
        from mtlora_amd import functional as Fn
        n = self.n
        res = [inp[f"res{k}"].to(dev()).requires_grad_(True) for k in range(1 if self.shared else n)]
        ys = [inp[f"y{k}"].to(dev()).requires_grad_(True) for k in range(n)]
        outs = Fn.ResidualDropPathFn.apply(_scale_kept(n, self.B).to(dev()), self.shared, n, *res, *ys)
        torch.autograd.backward(list(outs), [inp[f"g{k}"].to(dev()) for k in range(n)])
        r = {f"out{k}": outs[k] for k in range(n)}
        r.update({f"dy{k}": ys[k].grad for k in range(n)})
        r.update({f"dres{k}": t.grad for k, t in enumerate(res)})
        return r


class ConcatUpsampleCase(Case):
    B, H, W, chans = 2, 16, 24, (18, 36, 72, 144)

    def __init__(self, dtype):
        self.dtype = dtype
        self.key = f"concat_upsample-{dtype}"

    def layout(self):
        offs, at = [], 0
        for c in self.chans:  # (functional._pad4: every map starts on a 4-channel boundary, the row on an 8-channel one)
            offs.append(at)
            at += (c + 3) // 4 * 4
        return offs, (at + 7) // 8 * 8

    def make_inputs(self, gen):
        B, H, W = self.B, self.H, self.W
        offs, ld = self.layout()
        inp = {f"m{i}": _rnd((B, H >> i, W >> i, c), gen, self.dtype) for i, c in enumerate(self.chans)}
        inp["g"] = _rnd((B * H * W, ld), gen, self.dtype)
        return inp

    def poisons(self):
        B, H, W = self.B, self.H, self.W
        offs, ld = self.layout()
        every = ["out"] + [f"dm{i}" for i in range(4)]
        row = lambda b, i, j: (b * H + i) * W + j
        # INTERIOR fine pixels (at the border ATen's clamped second tap gets weight 0, and 0 * NaN is not generic)
        return [Poison("g", (row(0, 5, 6), offs[1] + 3), local=every), Poison("g", (row(B - 1, 10, 13), offs[3] + 143), local=every),
                Poison("g", (row(1, 7, 9), offs[2]), local=every), Poison("g", (row(0, 3, 3), offs[0] + 17), local=every),
                Poison("m2", (1, 2, 3, 71), local=every), Poison("m0", (0, 0, 0, 0), local=every)]

    def reference(self, inp):
        B, H, W = self.B, self.H, self.W
        offs, ld = self.layout()
        maps = [_d(inp[f"m{i}"]) for i in range(4)]
        ups = [maps[0]] + [F.interpolate(r.permute(0, 3, 1, 2), (H, W), mode="bilinear").permute(0, 2, 3, 1) for r in maps[1:]]
        out = torch.zeros(B, H, W, ld, dtype=torch.float64)
        g3 = inp["g"].double().view(B, H, W, ld)
        for o, c, u in zip(offs, self.chans, ups):
            out[..., o:o + c] = u.detach()
        sum((u * g3[..., o:o + c]).sum() for o, c, u in zip(offs, self.chans, ups)).backward()
        r = {"out": out.view(B * H * W, ld)}
        r.update({f"dm{i}": m.grad for i, m in enumerate(maps)})
        return r

    def run(self, inp):
        from mtlora_amd import functional as Fn
        maps = [inp[f"m{i}"].to(dev()).requires_grad_(True) for i in range(4)]
        out = Fn.ConcatUpsampleFn.apply(*maps)
        assert Fn.ConcatUpsampleFn.layout(list(self.chans)) == self.layout()
        out.backward(inp["g"].to(dev()))
        r = {"out": out}
        r.update({f"dm{i}": m.grad for i, m in enumerate(maps)})
        return r


GLUE_CASES = {f"droppath-shared{int(s)}-{str(y)[6:]}": DropPathCase(s, r, y) for s in (True, False) for r, y in LN_DTYPES}
GLUE_CASES.update({f"concat_upsample-{str(dt)[6:]}": ConcatUpsampleCase(dt) for dt in (F16, BF16)})


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", list(GLUE_CASES))
def test_residual_and_upsample_nonfinite(case, value):
    check_contract(GLUE_CASES[case], value)


def test_concat_upsample_pad_channels_stay_zero():
    """a poisoned fine gradient changes at most the 4 coarse pixels that tap it, in its own channel; the pad channels of the output
    stay zero whatever is poisoned"""
    case = GLUE_CASES["concat_upsample-float16"]
    offs, ld = case.layout()
    used = torch.zeros(ld, dtype=torch.bool)
    for o, c in zip(offs, case.chans):
        used[o:o + c] = True
    for p in case.poisons():
        masks = case.masks(p, NAN)
        if p.name == "g":
            for i in range(4):
                m = masks[f"dm{i}"]
                assert int(m.sum()) <= 4 and int(m.any(0).any(0).any(0).sum()) <= 1, (p, i, int(m.sum()))
        out = case.run(case.poisoned(p, NAN))["out"].cpu()
        assert (out[:, ~used] == 0).all(), p


ALL_CASES = [*LINEAR_CASES.values(), *MLP_CASES.values(), *LN_CASES.values(), *BN_CASES.values(), *ATTN_CASES.values(), *GLUE_CASES.values()]


# ------------------------------------------------------------------------------------------------
# genuine fp16 overflow, no injection: finite inputs whose exact result leaves the fp16 range
# ------------------------------------------------------------------------------------------------
def overflow_sets(ref64):
    """(where the fp64 result rounded to fp16 is inf, which elements are compared): elements whose magnitude lies within 10 % of 65504
    are left out (accumulation order decides those), at most 1 % of the tensor -- asserted from the reference alone"""
    ref64 = ref64.detach().double().cpu()
    assert torch.isfinite(ref64).all()
    band = (ref64.abs() > 0.9 * F16_MAX) & (ref64.abs() < 1.1 * F16_MAX)
    expect = torch.isinf(ref64.to(F16))
    assert band.float().mean().item() <= 0.01, f"{band.float().mean().item():.4f} of the tensor lies within 10 % of 65504"
    assert bool((expect & ~band).any()), "the case does not overflow"
    assert bool((~expect & ~band).any())
    return expect, ~band


def check_overflow(got, ref64, what):
    expect, cmp_ = overflow_sets(ref64)
    got = got.detach().cpu()
    assert got.dtype == F16, (what, got.dtype)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} NaN"
    wrong = (torch.isinf(got) != expect) & cmp_
    sat = int((wrong & expect).sum())
    assert not wrong.any(), f"{what}: {sat} elements finite where the fp16 result is inf (saturated), {int(wrong.sum()) - sat} inf where it is finite"
    assert torch.equal(torch.sign(got.float())[expect & cmp_], torch.sign(ref64.detach().cpu().float())[expect & cmp_]), what


class LinearOverflow:
    """y and dX of an MTLoRALinear whose row ``m`` of x / gy is scaled so that max |y[m]| / max |dX[m]| is 2e5 (pretrained weights of
    order 0.5 and small factors: the rank-space intermediates stay far inside the fp16 range)"""
    M, K, N, m = 130, 96, 160, 64

    def __init__(self):
        gen = torch.Generator().manual_seed(99)
        self.params = {"linear.weight": _rnd((self.N, self.K), gen, F16, 0.5).float(), "linear.bias": _rnd((self.N,), gen, F16, 0.5).float(),
                       "lora_shared_A": _rnd((16, self.K), gen, F16, 0.01).float(), "lora_shared_B": _rnd((self.N, 16), gen, F16, 0.01).float()}
        self.x, self.gy = _rnd((self.M, self.K), gen, F16), _rnd((self.M, self.N), gen, F16)
        y, dx = self.reference()
        self.x[self.m] = (self.x[self.m].double() * (2e5 / y[self.m].abs().max())).to(F16)
        self.gy[self.m] = (self.gy[self.m].double() * (2e5 / dx[self.m].abs().max())).to(F16)
        assert torch.isfinite(self.x).all() and torch.isfinite(self.gy).all()

    def reference(self):
        P = {n: v.double() for n, v in self.params.items()}
        x = _d(self.x)
        y, _ = O.mtlora_linear(x, P["linear.weight"], P["linear.bias"], P["lora_shared_A"], P["lora_shared_B"], 2.0)
        y.backward(self.gy.double())
        return y.detach(), x.grad

    def run(self):
        from mtlora_amd.lora import MTLoRALinear
        m = MTLoRALinear(self.K, self.N, r={"shared": 16}, lora_shared_scale=2.0, lora_dropout=0.0)
        m.load_state_dict(self.params)
        m = m.to(dev())
        x = self.x.to(dev()).requires_grad_(True)
        y, _ = m(x, None)
        y.backward(self.gy.to(dev()))
        return y, x.grad


class LayerNormOverflow:
    """gamma = 1e6 on every 24th column: |y| there is far past 65504 (but for |xhat| < 0.072), of order one elsewhere"""
    M, C = 65, 96

    def __init__(self):
        gen = torch.Generator().manual_seed(98)
        self.x, self.w, self.b = _rnd((self.M, self.C), gen, F16, 2.0, 0.5), _rnd((self.C,), gen, F32, 0.2, 1.0), _rnd((self.C,), gen, F32, 0.1)
        self.w[::24] = 1e6

    def reference(self):
        return F.layer_norm(self.x.double(), (self.C,), self.w.double(), self.b.double(), 1e-5)

    def run(self):
        from mtlora_amd import functional as Fn
        return Fn.LayerNormFn.apply(self.x.to(dev()), self.w.to(dev()), self.b.to(dev()), 1e-5, F16)


class DropPathOverflow:
    """6e4 + 6e4 (and -6e4 - 6e4) in two columns, order one elsewhere"""
    B, L, C = 2, 49, 96

    def __init__(self):
        gen = torch.Generator().manual_seed(97)
        self.res, self.y = _rnd((self.B, self.L, self.C), gen, F16), _rnd((self.B, self.L, self.C), gen, F16)
        self.res[..., 0] = self.y[..., 0] = 6e4
        self.res[..., self.C - 1] = self.y[..., self.C - 1] = -6e4

    def reference(self):
        return self.res.double() + self.y.double()

    def run(self):
        from mtlora_amd import functional as Fn
        return Fn.ResidualDropPathFn.apply(torch.ones(1, self.B, device=dev()), False, 1, self.res.to(dev()), self.y.to(dev()))[0]


class UpsampleOverflow(ConcatUpsampleCase):
    """fine gradients of 3e4 (+- 10 %) in half of the channels of the scale-2 map: each coarse pixel sums four or more of them"""

    def __init__(self):
        super().__init__(F16)
        inp = dict(self.inputs())
        offs, ld = self.layout()
        g = inp["g"].clone()
        half = self.chans[1] // 2  # (the other half keeps its order-one gradients: finite results next to the infinite ones)
        blk = g[:, offs[1]:offs[1] + half]
        g[:, offs[1]:offs[1] + half] = (3e4 * (1 + 0.1 * blk.float().clamp(-1, 1))).to(F16)
        inp["g"] = g
        self.inp = inp

    def reference_grad(self):
        return ConcatUpsampleCase.reference(self, self.inp)["dm1"]

    def run_grad(self):
        return ConcatUpsampleCase.run(self, self.inp)["dm1"]


OVERFLOW = {"linear": LinearOverflow, "layernorm": LayerNormOverflow, "droppath": DropPathOverflow, "upsample": UpsampleOverflow}


def overflow_reference(kind):
    """{output name: fp64 reference} of one overflow case (CPU only)"""
    c = OVERFLOW[kind]()
    if kind == "linear":
        y, dx = c.reference()
        return c, {"y": y, "dx": dx}
    if kind == "upsample":
        return c, {"dm1": c.reference_grad()}
    return c, {"out": c.reference()}


def test_linear_fp16_overflow_is_inf():
    c, ref = overflow_reference("linear")
    y, dx = c.run()
    check_overflow(y, ref["y"], "MTLoRALinear y")
    check_overflow(dx, ref["dx"], "MTLoRALinear dX")


def test_layernorm_fp16_overflow_is_inf():
    c, ref = overflow_reference("layernorm")
    check_overflow(c.run(), ref["out"], "LayerNorm y")


def test_residual_droppath_fp16_overflow_is_inf():
    c, ref = overflow_reference("droppath")
    check_overflow(c.run(), ref["out"], "ResidualDropPath out")


def test_concat_upsample_fp16_overflow_is_inf():
    c, ref = overflow_reference("upsample")
    check_overflow(c.run_grad(), ref["dm1"], "ConcatUpsample coarse gradient")


# ------------------------------------------------------------------------------------------------
# end to end: a loss scale that overflows the fp16 backward skips the step
# ------------------------------------------------------------------------------------------------
OVERFLOW_SCALE = 2.0 ** 40


def test_overflowing_scale_skips_the_step():
    """The model of test_fp16_autocast_train_steps_with_grad_scaler at a loss scale of 2^40.  Precondition from ATen alone: the fp32
    gradient of the plain MultiTaskLoss w.r.t. the low-resolution logits, times the scale, exceeds 65504.  Then with torch's GradScaler
    and with LossScaler + FusedAdamW.clip_and_step: a non-finite gradient arrives, nothing is updated (bitwise), the scale backs off --
    and the next step at the passing test's scale (1024) is applied."""
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW, LossScaler
    tasks = ["semseg", "normals", "sal", "human_parts"]
    img, tg = H.synthetic_batch(2, 224, tasks, seed=23, device=dev())

    def fresh(impl):
        torch.manual_seed(11)
        Fn._seed_counter = 0
        Fn.droppath_reset()
        model = H.build_model(img_size=224, tasks=tasks, depths=(2, 2, 2, 2), r_shared=16, r_task=4, drop_path_rate=0.0, seed=6,
                              DROPOUT=[0.0] * 4).to(dev()).train()
        return model, H.MultiTaskLoss(tasks), H.build_optimizer(model, lr=1e-3, impl=impl)

    def snap(model, opt):
        ps = [p.detach().clone() for p in model.parameters()]
        st = [v.detach().clone() for s in opt.state.values() for v in s.values() if isinstance(v, torch.Tensor)]
        return ps, st

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))

    def scaled_backward(model, crit, scale_fn):
        with torch.autocast("cuda", dtype=F16):
            loss, _ = crit.forward_low(model(img, upsample=False), tg)
        assert torch.isfinite(loss).all()
        scale_fn(loss).backward()

    # precondition (ATen only): the scaled gradient entering the heads' backward overflows fp16
    model, crit, opt = fresh("torch")
    with torch.no_grad(), torch.autocast("cuda", dtype=F16):
        low = model(img, upsample=False)
    low32 = {t: low[t].detach().float().requires_grad_(True) for t in tasks}
    pred = {t: F.interpolate(low32[t].permute(0, 3, 1, 2), size=tg[t].shape[-2:], mode="bilinear") for t in tasks}
    total, _ = crit(pred, tg)
    total.backward()
    gmax = max(low32[t].grad.abs().max().item() for t in tasks)
    assert gmax * OVERFLOW_SCALE > F16_MAX, (gmax, gmax * OVERFLOW_SCALE)

    # torch.amp.GradScaler
    scaler = torch.amp.GradScaler("cuda", init_scale=OVERFLOW_SCALE)
    before = snap(model, opt)
    scaled_backward(model, crit, scaler.scale)
    scaler.unscale_(opt)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and any(not torch.isfinite(g).all() for g in grads), "the overflow did not reach a parameter gradient"
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == OVERFLOW_SCALE * scaler.get_backoff_factor()
    assert same(before[0], snap(model, opt)[0]), "a skipped step changed a parameter"
    opt.zero_grad(set_to_none=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    scaled_backward(model, crit, scaler.scale)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() >= 1024.0
    assert not same(before[0], snap(model, opt)[0]), "the step at scale 1024 was skipped"

    # LossScaler + FusedAdamW
    model, crit, opt = fresh("hip")
    assert isinstance(opt, FusedAdamW)
    ls = LossScaler(init_scale=1024.0)
    scaled_backward(model, crit, ls.scale)  # (one applied step first: the optimizer state exists and must stay as it is)
    opt.clip_and_step(max_norm=5.0, scaler=ls)
    opt.zero_grad(set_to_none=True)
    assert ls.get_scale() >= 1024.0
    ls = LossScaler(init_scale=OVERFLOW_SCALE)
    before = snap(model, opt)
    assert before[1], "no optimizer state"
    scaled_backward(model, crit, ls.scale)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and any(not torch.isfinite(g).all() for g in grads)
    norm = opt.clip_and_step(max_norm=5.0, scaler=ls)
    assert not math.isfinite(norm.item())  # found_inf: the norm of the unscaled gradients is not finite
    assert ls.get_scale() == OVERFLOW_SCALE * 0.5
    after = snap(model, opt)
    assert same(before[0], after[0]) and same(before[1], after[1]), "a skipped step changed parameters or optimizer state"
    opt.zero_grad(set_to_none=True)
    ls = LossScaler(init_scale=1024.0)
    scaled_backward(model, crit, ls.scale)
    opt.clip_and_step(max_norm=5.0, scaler=ls)
    assert ls.get_scale() >= 1024.0
    assert not same(before[0], snap(model, opt)[0]), "the step at scale 1024 was skipped"
