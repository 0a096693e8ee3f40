"""torch.autograd.Function wrappers over the C ABI (include/mtlora_hip.h).

Host-side plumbing only: allocate outputs / ctx / scratch with torch, pass raw pointers and the
current stream to the library.  Every op raises if the library or a GPU tensor is missing.
"""
from __future__ import annotations

import ctypes
import os
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from . import _lib as L

# ----------------------------------------------------------------------------------------------
# dropout seeds: one fresh 64-bit seed per MTLoRALinear call in training mode, derived from
# torch.initial_seed() and a call counter (deterministic under torch.manual_seed + fixed call order)
# ----------------------------------------------------------------------------------------------
_seed_counter = 0


# optional device-resident offset added to every dropout seed when the kernels RUN (mtlora_linear_desc.seed_offset):
# a captured HIP graph bakes the host-side seeds in, so a graphed train step bumps this one int64 between replays.
_seed_offset: Optional[torch.Tensor] = None


def set_seed_offset(t: Optional[torch.Tensor]) -> None:
    """install (or clear) the device int64[1] tensor whose value is added to the dropout seeds at kernel time."""
    global _seed_offset
    if t is not None and not (t.is_cuda and t.dtype == torch.int64 and t.numel() == 1):
        raise RuntimeError("mtlora_amd: the seed offset must be a CUDA int64 tensor with one element")
    _seed_offset = t


# optional second stream for the factor gradients (dA_*, dB_*: the split-M k_tn reductions) of MTLoRALinear.backward:
# nothing in the backward chain depends on them (only the optimizer / the gradient reducer does), and they are a fifth of
# the linear path's kernel time, mostly as latency-bound launches -- on their own stream they fill the gaps of the main
# chain.  The caller that installs a stream must JOIN it before the gradients are read (train_step does; a GradReducer gets
# it through ``extra_streams``).  Off (None) by default: a plain ``loss.backward()`` stays single-stream.
_factor_stream: Optional["torch.cuda.Stream"] = None
# layers with fewer rows than this keep their factor gradients on the main stream: the fork / join costs ~30 us of host time per
# layer and only pays while the kernels are long enough for the GPU to be the bottleneck (C1 at batch 2, M <= 6272 everywhere,
# ran 35 % SLOWER with the side stream: 18.7 vs 13.8 ms / step)
_FACTOR_MIN_M = int(os.environ.get("MTLORA_FACTOR_MIN_M", "8192"))


# factor parameters whose gradient was written on the side stream by an earlier backward call -> (that stream, the autograd graph
# task it happened in).  A later use of the same layer makes its own stream WAIT for the side stream before anything touches the
# gradient; whether the side stream may be used again depends on WHEN the entry was written:
#   * in the CURRENT backward pass (the layer is applied twice in one graph): the autograd engine sums the two gradients of a factor
#     on the stream of the forward call, so the second gradient stays on that stream;
#   * in an EARLIER pass that nobody joined: once waited for, the side stream is free again (unless the factor's .grad exists, in
#     which case autograd accumulates into it on this stream -- ``use_side`` checks that separately).
# Keys are compared by IDENTITY (a WeakKeyDictionary compares its referents with ``==``, which is element-wise for
# tensors -- looking up a present key raised "Boolean value of Tensor ... is ambiguous"); weak, so a freed Parameter leaves no
# entry behind (raw ids can be reused by other objects).  A caller that joins the side stream AFTER the backward pass (train_step,
# GraphedTrainStep) says so with ``factor_stream_joined()``; the GradReducer's mid-pass waits do not (the same-pass rule above
# must keep holding for the rest of the pass).
from torch.utils.weak import WeakIdKeyDictionary  # noqa: E402

_side_pending: "WeakIdKeyDictionary" = WeakIdKeyDictionary()


def factor_stream_joined() -> None:
    """the caller made its stream wait for the side stream: nothing written there is pending any more"""
    _side_pending.clear()


def set_factor_stream(stream: Optional["torch.cuda.Stream"]) -> None:
    """install (or, with None, remove) the side stream for the factor gradients (see above).  Entries of ``_side_pending`` stay:
    whoever installs / removes the stream has not necessarily joined the previous one (``factor_stream_joined`` says that)."""
    global _factor_stream
    _factor_stream = stream


def _graph_task_id() -> int:
    return torch._C._current_graph_task_id()


def _side_join_pending(params, dev) -> bool:
    """make the current stream wait for every side stream that still holds a gradient of ``params`` (the layer's factor
    Parameters) from an earlier backward call.  Returns True when one of those entries was written in the CURRENT backward pass
    (same layer twice in one graph): this call's factor gradients must then stay on the current stream."""
    if not _side_pending:
        return False
    same_pass, streams, task = False, {}, _graph_task_id()
    for p in params:
        if p is None:
            continue
        ent = _side_pending.pop(p, None)
        if ent is not None:
            streams[id(ent[0])] = ent[0]
            same_pass = same_pass or ent[1] == task
    cur = torch.cuda.current_stream(dev) if streams else None
    for st in streams.values():
        cur.wait_stream(st)
    if same_pass:
        # a THIRD (fourth ...) use of the layer in this pass must see the same-pass rule too -- the entries popped above are
        # put back under the current graph task, so every later use keeps its factor gradients on the stream autograd sums them on
        side = next(iter(streams.values()))
        for p in params:
            if p is not None:
                _side_pending[p] = (side, task)
    return same_pass


def _side_safe_params(params) -> bool:
    """may the gradients of ``params`` be WRITTEN on the side stream?  Only when autograd will take the gradient tensor as it is:
    no existing .grad to accumulate into (an add on the backward's stream), no tensor hook on the Parameter (a hook receives --
    and may replace, i.e. force a copy of -- the gradient on the backward's stream while the side stream is still writing it) and
    no NON-LEAF factor (lora.py's rank-aware Delta W: its producer's backward reads the gradient on the backward's stream)."""
    return all(p is None or (p.grad is None and not p._backward_hooks and (p.is_leaf or not p.requires_grad)) for p in params)


def _side_mark_pending(params, side) -> None:
    task = _graph_task_id()
    for p in params:
        if p is not None:
            _side_pending[p] = (side, task)


def factor_stream() -> Optional["torch.cuda.Stream"]:
    return _factor_stream


def _run_factor_phases(params, fgrads, M: int, dev, extra_ok: bool, run, keep) -> None:
    """a node's backward launches, ``run(phase, stream_ptr)`` with the library's ``bwd_phase`` meaning (0 all, 1 the chain, 2 the
    factor gradients): ``run(0)`` here, or ``run(1)`` here, an event and ``run(2)`` on the side stream, which then holds the gradients
    of ``params``; ``keep()`` lists what phase 2 touches.  ``extra_ok``: nothing in this backward reads ``fgrads`` on this stream."""
    side = _factor_stream
    use_side = (side is not None and bool(fgrads) and extra_ok and side.device == dev and M >= _FACTOR_MIN_M
                and _side_safe_params(params))
    if _side_join_pending(params, dev):
        use_side = False  # same layer earlier in THIS backward pass: autograd sums the two gradients on this stream
    if not use_side:
        run(0, L.stream_ptr())
        return
    run(1, L.stream_ptr())
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    run(2, ctypes.c_void_p(side.cuda_stream))
    _side_mark_pending(params, side)
    for t in keep():
        t.record_stream(side)


# ----------------------------------------------------------------------------------------------
# DropPath keep / scale vectors, drawn in bulk.  Every residual of the backbone needs n x B per-sample factors
# bernoulli(keep) / keep (timm DropPath, swin_transformer_mtlora.py:388-426): 22 draws per Swin-T step = 44 tiny launches
# (bernoulli_, div_) strung along the forward's critical path.  A train step can announce itself (``droppath_begin_step`` /
# ``droppath_end_step``, mtl_harness.train_step): the sequence of requests (n, B, keep) seen in one step is replayed as the PLAN of
# the next one, whose factors then come from ONE rand + compare + scale over all of them; a request that deviates from the plan
# (other model, other batch, eval) simply draws on its own and the plan is re-recorded.  Same distribution, same global CUDA
# generator; the individual values differ from per-call draws.
# ----------------------------------------------------------------------------------------------
class _DropPathPool:
    def __init__(self):
        self.plan, self.rec, self.rows, self.at, self.active, self.in_step = [], [], None, 0, False, False
        self.cache_key, self.keep_col = None, None

    def begin(self, device):
        self.rec, self.at, self.in_step = [], 0, True
        capturing = torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()
        self.active = bool(self.plan) and not capturing
        if not self.active:
            return
        key = (tuple(self.plan), str(device))
        if key != self.cache_key:  # per-row keep probabilities of the plan (built once)
            B = self.plan[0][1]
            if any(b != B for _, b, _ in self.plan):
                self.active = False
                return
            keeps = [k for n, _, k in self.plan for _ in range(n)]
            self.keep_col = torch.tensor(keeps, dtype=torch.float32, device=device).unsqueeze(1)
            self.cache_key = key
        B = self.plan[0][1]
        u = torch.rand(self.keep_col.shape[0], B, dtype=torch.float32, device=device)
        self.rows = (u < self.keep_col) / self.keep_col  # bernoulli(keep) / keep, all requests of the step at once
        self.off = 0

    def end(self):
        if self.in_step:
            self.plan, self.in_step, self.active, self.rows = self.rec, False, False, None

    def scale(self, n: int, B: int, keep: float, device) -> torch.Tensor:
        if self.in_step:
            self.rec.append((n, B, keep))
            if self.active and self.at < len(self.plan) and self.plan[self.at] == (n, B, keep) and self.rows.device == device:
                out = self.rows[self.off:self.off + n]
                self.off += n
                self.at += 1
                return out
            self.active = False
        return torch.empty(n, B, dtype=torch.float32, device=device).bernoulli_(keep).div_(keep)


_droppath_pool = _DropPathPool()


def droppath_begin_step(device) -> None:
    _droppath_pool.begin(device)


def droppath_end_step() -> None:
    _droppath_pool.end()


def droppath_reset() -> None:
    """forget the recorded plan: the next announced step draws per request again (two runs that must see the same random
    stream have to start from the same pool state)."""
    global _droppath_pool
    _droppath_pool = _DropPathPool()


def droppath_scale(n: int, B: int, keep: float, device) -> torch.Tensor:
    """(n, B) fp32 factors bernoulli(keep) / keep -- from the step's bulk draw when one is active (see _DropPathPool)."""
    return _droppath_pool.scale(n, B, keep, device)


# ----------------------------------------------------------------------------------------------
# kernel selection (mtlora_linear_desc.sel_* / max_cu, ABI v6).  The LIBRARY reads no environment variables; this module reads
# the developer switches once at import and hands them to every call through the descriptor.  ``set_tuning`` overrides them in
# process (tests: the "[tiled]" / "[dense]" / "[persist]" families of tests/conftest.py; tools/bench_linear.py A/B runs).
#   MTLORA_SP=0        -> stream=1  (tiled kernels only)         MTLORA_NTD=0 / 2      -> dense=1 / 2 (k_ntd never / whenever)
#   MTLORA_SP_TN=0 / 2 -> tn=1 / 2  (k_sp_tn never / whenever)   MTLORA_SP_PROJK=0 / 2 -> projk=1 / 2
#   MTLORA_MAX_CU=n    -> max_cu=n  (persistent grids sized as if the device had n CUs)
# ----------------------------------------------------------------------------------------------
def _env_tri(name: str) -> int:
    v = os.environ.get(name)
    return 0 if v is None or v == "1" else (1 if v == "0" else int(v))


_TUNING_DEFAULT = {"stream": 1 if os.environ.get("MTLORA_SP") == "0" else 0, "dense": _env_tri("MTLORA_NTD"),
                   "tn": _env_tri("MTLORA_SP_TN"), "projk": _env_tri("MTLORA_SP_PROJK"),
                   "max_cu": int(os.environ.get("MTLORA_MAX_CU", "0"))}
_tuning = dict(_TUNING_DEFAULT)


def set_tuning(**kw) -> dict:
    """override kernel-selection switches for the calls that follow (keys: stream, dense, tn, projk, max_cu; values as in
    include/mtlora_hip.h: 0 = library default); ``set_tuning()`` with no arguments restores the import-time values.
    Returns the previous settings."""
    prev = dict(_tuning)
    if not kw:
        _tuning.update(_TUNING_DEFAULT)
    for k, v in kw.items():
        if k not in _tuning:
            raise KeyError(f"mtlora_amd: unknown tuning key {k!r} (have {sorted(_tuning)})")
        _tuning[k] = int(v)
    return prev


def next_seed() -> int:
    global _seed_counter
    _seed_counter += 1
    x = (torch.initial_seed() * 0x9E3779B97F4A7C15 + _seed_counter * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 31
    return x & 0xFFFFFFFFFFFFFFFF


_HOT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_GLUE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)  # LayerNorm family, residual + DropPath, BatchNorm + ReLU kernels


def compute_dtype(x: torch.Tensor) -> torch.dtype:
    """dtype the hot path (MTLoRALinear, window attention) runs in: the autocast dtype when autocast is on (like F.linear),
    else x's.  bf16 is the dtype to use on MI355X (same MFMA rate as fp16, no loss scaling); fp16 -- the reference's
    ``torch.cuda.amp.autocast()`` default, main.py:341 -- is supported by the linear / attention kernels, with the block glue
    (LayerNorm, residuals, heads) falling back to fp32 outputs / ATen for it."""
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda")
        if dt not in _HOT_DTYPES:
            raise RuntimeError(f"mtlora_amd: unsupported autocast dtype {dt}")
        return dt
    if x.dtype not in _HOT_DTYPES:
        raise RuntimeError(f"mtlora_amd: unsupported activation dtype {x.dtype}")
    return x.dtype


def glue_dtype(x: torch.Tensor) -> torch.dtype:
    """output dtype of the fused glue kernels in front of an MTLoRALinear: the compute dtype (fp32, or bf16 / fp16 under
    autocast -- the LayerNorm-family, residual and BatchNorm kernels are instantiated for all three)."""
    return compute_dtype(x)


# ----------------------------------------------------------------------------------------------
# MTLoRALinear
# ----------------------------------------------------------------------------------------------
@dataclass
class LinearMeta:
    """static description of one MTLoRALinear call (lora.py:253-284)."""
    K: int
    N: int
    r_s: int
    r_t: Tuple[int, ...]
    scale_s: Union[float, torch.Tensor]               # a float, or the 1-element fp32 device tensor of a TRAINABLE scale (the Parameter):
    scale_t: Tuple[Union[float, torch.Tensor], ...]   # such a segment is packed from device memory, the descriptor then carries 1.0
    mode: int                 # 0 matrix, 1 matrixv2
    has_x_tasks: bool
    dropout_p: float          # 0 in eval
    seed: int
    dtype: torch.dtype
    weight_requires_grad: bool = False
    n_scale_t: int = 0        # >0: per-task scales are trainable Parameters passed after B_t
    n_gate: int = 0           # >0: x (and x_t) = gelu(gate): the LAST n_gate args are the pre-activations; dx *= gelu'(gate)
    gelu_out: bool = False    # also return gelu(y) for every output (fc1 of the Mlp): outputs = (y_s, *y_t, a_s, *a_t)
    packed: Optional[torch.Tensor] = None  # the layer's factors packed ahead of time (PackTable / mtlora_linear_pack): fwd skips k_pack

    @property
    def T(self) -> int:
        return len(self.r_t)

    @property
    def scale_dev(self):
        """None when every scale is a constant, else the 1 + T list (shared, tasks) of the scale tensors, None where constant"""
        if not (isinstance(self.scale_s, torch.Tensor) or any(isinstance(v, torch.Tensor) for v in self.scale_t)):
            return None
        return [v if isinstance(v, torch.Tensor) else None for v in (self.scale_s, *self.scale_t)]

    def desc(self, M: int) -> L.LinearDesc:
        d = L.LinearDesc()
        d.M, d.K, d.N = M, self.K, self.N
        d.dtype = L._DT[self.dtype]
        d.mode, d.T, d.r_s = self.mode, self.T, self.r_s
        for i, r in enumerate(self.r_t):
            d.r_t[i] = r
            d.scale_t[i] = 1.0 if isinstance(self.scale_t[i], torch.Tensor) else self.scale_t[i]
        # (a device scale only enters through the packed factors; a call with d.packed set never reads d.scale_*: include/mtlora_hip.h)
        d.scale_s = 1.0 if isinstance(self.scale_s, torch.Tensor) else self.scale_s
        d.has_x_tasks = 1 if self.has_x_tasks else 0
        d.dropout_p = self.dropout_p
        d.seed = self.seed
        d.seed_offset = 0 if _seed_offset is None else _seed_offset.data_ptr()
        tu = _tuning
        d.sel_stream, d.sel_dense, d.sel_tn, d.sel_projk, d.max_cu = tu["stream"], tu["dense"], tu["tn"], tu["projk"], tu["max_cu"]
        d.packed = 0 if self.packed is None else self.packed.data_ptr()
        return d


def _flat(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """t itself when it is already contiguous in ``dtype`` (the kernels take a pointer and a row count: no 2-D view object is needed --
    each ``.view`` costs ~1.5 us of dispatch, 10 of them per MTLoRALinear call), else a contiguous copy in ``dtype``"""
    if t.dtype == dtype and t.is_contiguous():
        return t
    return t.to(dtype).contiguous()


def _f32c(p):
    """fp32 contiguous view of a factor (Parameters already are: used as they come, autograd is off inside Function.forward)."""
    if p is None or (p.dtype == torch.float32 and p.is_contiguous()):
        return p
    return p.detach().float().contiguous()


def _f32_param(t: torch.Tensor) -> torch.Tensor:
    """a parameter as the glue kernels read it (LayerNorm / BatchNorm affine, attention bias): detached, fp32, contiguous"""
    return t.detach().float().contiguous()


def _scratch(nbytes: int, device, what: str, *dims, floor: int = 0) -> torch.Tensor:
    """the uint8 buffer of a size query's answer, at least ``floor`` bytes; a negative answer refuses the shape ``dims`` of ``what``"""
    if nbytes < 0:
        raise RuntimeError(f"mtlora_amd: invalid {what} {dims}")
    return torch.empty(nbytes if nbytes > floor else floor, dtype=torch.uint8, device=device)


# size queries of the linear family, cached: one ctypes call per new descriptor, whatever the query
_D = L.LinearDesc
# the key's four runs of bytes -- [M, K, N, dtype, mode, T, r_s, r_t] [has_x_tasks] [sel_stream, sel_dense, sel_tn, sel_projk, max_cu]
# [hid] -- cut out of the struct by ONE unpack (the buffer protocol of ctypes structures; the cheapest way found to read 20 fields)
_KEY_CUT = struct.Struct(f"{_D.scale_s.offset}s{_D.has_x_tasks.offset - _D.scale_s.offset}x4s{_D.sel_stream.offset - _D.has_x_tasks.offset - 4}x"
                         f"{_D.packed.offset - _D.sel_stream.offset}s{_D.hid.offset - _D.packed.offset}x4s"
                         f"{ctypes.sizeof(_D) - _D.hid.offset - 4}x").unpack
_size_cache: dict = {}


def _size_query(kind: str, fn, d, d2=None) -> int:
    """``fn(&d)`` / ``fn(&d, &d2)`` of a size (or yes / no) query of the library, asked once per ``kind`` (a name for ``fn``: ctypes
    functions do not hash) and key.  The key is cut out of the descriptor(s): every field but the pointers' values (seed_offset,
    hid_ptr; of ``packed`` only whether it is set), the per-call seed and bwd_phase, and the scales and dropout_p, which enter no
    size.  What csrc/linear.hip reads (check_desc, first in every query, only VALIDATES; a value out of range answers -1):
      ctx_layout (ctx bytes)                        M, K, N, dtype, T, r_s, r_t, packed != 0
      bwd_scratch with sp_tn_part_bytes             M, K, N, dtype, T, r_s, r_t
      hid_check (hid_supported, every hid query)    both: M, K, N, dtype, T, r_t, mode, has_x_tasks; d1.sel_stream
      hid_fwd_scratch_bytes / hid_bwd_part_bytes    d1: M, N, T, r_t, sel_stream, max_cu; d2: r_t
    A superset: mode, has_x_tasks, every sel_* and the hid flags are in the key of every query."""
    key = (kind, _KEY_CUT(d), d.packed is None) if d2 is None else (kind, _KEY_CUT(d), d.packed is None, _KEY_CUT(d2), d2.packed is None)
    v = _size_cache.get(key)
    if v is None:
        v = fn(ctypes.byref(d)) if d2 is None else fn(ctypes.byref(d), ctypes.byref(d2))
        _size_cache[key] = v
    return v


class PackTable:
    """ONE launch per optimizer step that packs the low-rank factors of many MTLoRALinear layers (``mtlora_linear_pack_table``).

    ``entries``: list of (meta, A_s, B_s, A_t list, B_t list, packed uint8 tensor) -- ``meta`` a LinearMeta carrying the scales,
    dropout_p and has_x_tasks the layer is CALLED with (they enter the alpha-scaled copies).  The table holds raw device pointers of
    the masters and the destinations: valid while those tensors live and are only updated in place (``nn.Parameter``s under an
    optimizer; the packed buffers are owned by the layers)."""

    def __init__(self, entries, device, dtype: torch.dtype):
        lib = L.lib()
        eb = lib.mtlora_linear_pack_entry_bytes()
        host = (ctypes.c_ubyte * (eb * max(len(entries), 1)))()
        self.keep = entries  # (keeps every tensor whose address is in the table alive)
        for i, (meta, A_s, B_s, A_t, B_t, packed, *_owner) in enumerate(entries):
            d = meta.desc(1)
            d.packed = 0
            sd = meta.scale_dev  # (trainable scales: the entry holds their addresses, the launch reads them when it runs)
            if sd is None:
                st = lib.mtlora_linear_pack_entry(ctypes.byref(d), L.ptr(A_s), L.ptr(B_s), L.ptr_array(A_t), L.ptr_array(B_t), L.ptr(packed),
                                                  packed.numel(), ctypes.byref(host, i * eb))
            else:
                st = lib.mtlora_linear_pack_entry_dev(ctypes.byref(d), L.ptr(A_s), L.ptr(B_s), L.ptr_array(A_t), L.ptr_array(B_t),
                                                      L.ptr_array9(sd), len(sd), L.ptr(packed), packed.numel(), ctypes.byref(host, i * eb))
            L.check(st, "mtlora_linear_pack_entry")
        self.n = len(entries)
        self.dtype_code = L._DT[dtype]
        self.table = torch.frombuffer(host, dtype=torch.uint8).clone().to(device)

    def pack(self) -> None:
        if self.n:
            L.check(L.lib().mtlora_linear_pack_table(L.ptr(self.table), self.n, self.dtype_code, L.stream_ptr()), "mtlora_linear_pack_table")


def packed_bytes(meta: "LinearMeta") -> int:
    d = meta.desc(1)
    d.packed = 0
    n = L.lib().mtlora_linear_packed_bytes(ctypes.byref(d))
    if n < 0:
        raise RuntimeError("mtlora_amd: invalid MTLoRALinear shape for mtlora_linear_packed_bytes")
    return n


def pack_dev(meta: "LinearMeta", A_s, B_s, A_t, B_t, buf: torch.Tensor) -> None:
    """one launch that packs a layer's factors into ``buf`` (``packed_bytes(meta)`` bytes), the trainable scales of ``meta`` read from
    device memory by the kernel (``mtlora_linear_pack_dev``): nothing is read back, and inside a capture every replay packs from the
    Parameters' current values"""
    sd = meta.scale_dev
    A_s, B_s, A_t, B_t = _f32c(A_s), _f32c(B_s), [_f32c(a) for a in A_t], [_f32c(b) for b in B_t]
    L.require_gpu(buf, A_s, B_s, *A_t, *B_t, *sd)
    if any(v is not None and (v.dtype != torch.float32 or v.numel() != 1) for v in sd):
        raise RuntimeError("mtlora_amd: a trainable LoRA scale must be a 1-element fp32 tensor")
    d = meta.desc(1)
    d.packed = 0
    st = L.lib().mtlora_linear_pack_dev(ctypes.byref(d), L.ptr(A_s), L.ptr(B_s), L.ptr_array(A_t), L.ptr_array(B_t), L.ptr_array9(sd),
                                        len(sd), L.ptr(buf), buf.numel(), L.stream_ptr())
    L.check(st, "mtlora_linear_pack_dev")


def scale_grad_torch(dB: torch.Tensor, B: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """portable definition of ``mtlora_linear_scale_grad`` for one segment: d(loss)/d(scale) = <dB, B> / scale (the output carries
    scale * B (..), so dB = scale * Z and d scale = <Z, B>), summed in double; 0 where the scale is 0.  Returns a 1-element fp32 tensor."""
    t = (dB.double() * B.double()).sum()
    sv = s.detach().double().reshape(())
    return torch.where(sv == 0, torch.zeros_like(t), t / torch.where(sv == 0, torch.ones_like(sv), sv)).float().reshape(1)


def weight_cast(w: torch.Tensor, wc: torch.Tensor, wt: torch.Tensor) -> None:
    """refill ``wc`` (N, K) and ``wt`` (K, N), contiguous and of one dtype, from the contiguous fp32 master ``w`` (N, K) in one launch
    (``mtlora_linear_weight_cast``): bit-equal to ``w.to(dtype)`` and its transpose.  A raw-pointer write: no version counter moves,
    so a buffer that an earlier call saved for backward stays usable, and a captured graph re-reads the master on every replay."""
    L.require_gpu(w, wc, wt)
    N, K = w.shape
    if (w.dtype != torch.float32 or not w.is_contiguous() or wc.dtype != wt.dtype or wc.shape != (N, K) or wt.shape != (K, N)
            or not wc.is_contiguous() or not wt.is_contiguous()):
        raise RuntimeError("mtlora_amd: weight_cast takes a contiguous fp32 (N, K) master and contiguous (N, K), (K, N) copies of one dtype")
    L.check(L.lib().mtlora_linear_weight_cast(L.ptr(w), N, K, L.dtype_code(wc), L.ptr(wc), L.ptr(wt), L.stream_ptr()),
            "mtlora_linear_weight_cast")


def weight_grad_torch(x: torch.Tensor, dys) -> torch.Tensor:
    """portable definition of ``mtlora_linear_weight_grad``: dW (N, K) = (sum of the output gradients)^T x for the shared input ``x``
    (..., K) of the dense product and the gradients ``dys`` (each (..., N), or None for an output that got none) of the 1 + T outputs,
    which all add the same x W^T + b (reference lora.py:255-284).  Computed in the dtype of ``x``; at least one gradient must be given."""
    x2 = x.reshape(-1, x.shape[-1])
    G = None
    for g in dys:
        if g is not None:
            g2 = g.reshape(x2.shape[0], -1).to(x2.dtype)
            G = g2 if G is None else G + g2
    if G is None:
        raise ValueError("weight_grad_torch: every output gradient is None")
    return G.t() @ x2


_SG_BYTES = None


def _scale_grad_bytes() -> int:
    global _SG_BYTES
    if _SG_BYTES is None:
        _SG_BYTES = L.lib().mtlora_linear_scale_grad_scratch_bytes()
    return _SG_BYTES


class MTLoRALinearFn(torch.autograd.Function):
    """(y_s, y_t[0..T-1]) = f(x, x_t[0..T-1], A_s, B_s, A_t[..], B_t[..]); W (and bias) frozen by default.

    args: meta, x, W_c, Wt_c, bias_f32, W_master, bias_master, A_s, B_s, scale_s_param,
          *x_t(T or 0), *A_t(T), *B_t(T), *scale_t_params(T or 0), *gelu_gates(0 or 1 + len(x_t))
    W_c / Wt_c are the compute-dtype copies the module caches; W_master / bias_master are only used to
    route gradients when the pretrained weight is left trainable (MTLORA.FREEZE_PRETRAINED False);
    scale_*_param are the 1-element Parameters of TRAINABLE_SCALE_* (None otherwise): the packing launch reads them on the
    device (``meta.packed`` is always set for such a layer) and d(loss)/d(scale) = <dB, B> / scale is formed from the factor
    gradient by ``mtlora_linear_scale_grad``, queued behind the factor gradients on whichever stream they run on."""

    @staticmethod
    def forward(ctx, meta: LinearMeta, x, W_c, Wt_c, bias_f32, W_master, bias_master, A_s, B_s, scale_s_param, *rest):
        ctx.set_materialize_grads(False)  # an unused output must reach backward as None, not as zeros
        T = meta.T
        nx = T if meta.has_x_tasks else 0
        x_t, A_t, B_t = list(rest[:nx]), list(rest[nx:nx + T]), list(rest[nx + T:nx + 2 * T])
        L.require_gpu(x, W_c, *x_t)
        lead = x.shape[:-1]
        x2 = _flat(x, meta.dtype)              # (M x K) row-major whatever the leading shape
        xt2 = [_flat(t, meta.dtype) for t in x_t]
        M = x2.numel() // meta.K
        if x2.shape[-1] != meta.K or any(t.shape != x2.shape for t in xt2):
            raise RuntimeError(f"mtlora_amd: MTLoRALinear input of shape {tuple(x.shape)} for in_features = {meta.K}")
        d = meta.desc(M)
        lib = L.lib()
        ctx_bytes = _size_query("ctx", lib.mtlora_linear_ctx_bytes, d)
        ctxbuf = _scratch(ctx_bytes, x.device, "MTLoRALinear shape (M, K, N; K and N must be multiples of 8)", M, meta.K, meta.N)
        oshape = (*lead, meta.N)
        ys = torch.empty(oshape, dtype=meta.dtype, device=x.device)
        yt = [torch.empty(oshape, dtype=meta.dtype, device=x.device) for _ in range(T)]
        A_s_c, B_s_c = _f32c(A_s), _f32c(B_s)
        A_t_c, B_t_c = [_f32c(a) for a in A_t], [_f32c(b) for b in B_t]
        acts = []
        if meta.gelu_out:  # second outputs gelu(y) written by the same epilogue (mtlora_linear_fwd_gelu)
            acts = [torch.empty(oshape, dtype=meta.dtype, device=x.device) for _ in range(1 + T)]
            st = lib.mtlora_linear_fwd_gelu(ctypes.byref(d), L.ptr(x2), L.ptr_array(xt2), L.ptr(W_c), L.ptr(bias_f32),
                                            L.ptr(A_s_c), L.ptr(B_s_c), L.ptr_array(A_t_c), L.ptr_array(B_t_c), L.ptr(ys),
                                            L.ptr_array(yt), L.ptr(acts[0]), L.ptr_array(acts[1:]), L.ptr(ctxbuf), ctx_bytes,
                                            L.stream_ptr())
            L.check(st, "mtlora_linear_fwd_gelu")
        else:
            st = lib.mtlora_linear_fwd(ctypes.byref(d), L.ptr(x2), L.ptr_array(xt2), L.ptr(W_c), L.ptr(bias_f32),
                                       L.ptr(A_s_c), L.ptr(B_s_c), L.ptr_array(A_t_c), L.ptr_array(B_t_c), L.ptr(ys),
                                       L.ptr_array(yt), L.ptr(ctxbuf), ctx_bytes, L.stream_ptr())
            L.check(st, "mtlora_linear_fwd")
        ctx.meta, ctx.lead, ctx.nx = meta, lead, nx
        ctx.in_dtypes = [x.dtype] + [t.dtype for t in x_t]
        gates = []
        if meta.n_gate:
            gates = list(rest[len(rest) - meta.n_gate:])
            if len(gates) != 1 + nx or any(g.dtype != meta.dtype or not g.is_contiguous() or g.numel() != x2.numel() or g.shape[-1] != meta.K
                                           for g in gates):
                raise RuntimeError("mtlora_amd: gelu gates must be contiguous pre-activations of x / x_t in the compute dtype")
        ctx.save_for_backward(x2, Wt_c, ctxbuf, *xt2, *gates)
        ctx.keep = (A_s_c, B_s_c, A_t_c, B_t_c)  # fp32 factor views (also used for the trainable-scale gradients)
        # (meta.packed keeps the packed-factor buffer alive until backward; a trainer overwrites it only after the step's backward)
        ctx.factor_params = (A_s, B_s, *A_t, *B_t)  # the Parameters themselves: backward looks at their .grad (side stream)
        ctx.has_scale_s = scale_s_param is not None
        if ctx.has_scale_s or meta.n_scale_t:
            if meta.packed is None or meta.scale_dev is None:
                raise RuntimeError("mtlora_amd: a layer with trainable scales runs from factors packed with mtlora_linear_pack_dev")
            ctx.factor_params += (scale_s_param, *rest[nx + 2 * T:nx + 2 * T + meta.n_scale_t])  # (their gradients: same stream)
        ctx.bias_param, ctx.weight_param = bias_master, W_master  # (trainable: their gradients run with the factor gradients, see backward)
        ctx.M = M
        return (ys, *yt, *acts)

    @staticmethod
    def backward(ctx, *grads):
        meta: LinearMeta = ctx.meta
        T, nx = meta.T, ctx.nx
        if meta.gelu_out:
            # a gradient arriving on a_k = gelu(y_k) comes from a consumer that already applied gelu'(y_k) (an MTLoRALinear
            # called with gelu_gate = y_k): it IS a gradient w.r.t. y_k
            gy, ga = grads[:1 + T], grads[1 + T:]
            grads = tuple(a if y is None else (y if a is None else y + a) for y, a in zip(gy, ga))
        if all(g is None for g in grads):
            return (None,) * (10 + nx + 2 * T + meta.n_scale_t + meta.n_gate)
        x2, Wt_c, ctxbuf, *xt2 = ctx.saved_tensors
        gates = []
        if meta.n_gate:
            xt2, gates = xt2[:nx], xt2[nx:]
        M = ctx.M
        dev = x2.device
        g2 = [None if g is None else _flat(g, meta.dtype) for g in grads]
        dy_s, dy_t = g2[0], g2[1:1 + T]
        d = meta.desc(M)
        lib = L.lib()
        scratch_bytes = _size_query("bwd", lib.mtlora_linear_bwd_scratch_bytes, d)
        scratch = _scratch(scratch_bytes, dev, "MTLoRALinear backward shape (M, K, N)", M, meta.K, meta.N)
        need = ctx.needs_input_grad  # (meta, x, W_c, Wt_c, bias_f32, W_master, bias_master, A_s, B_s, scale_s, *rest)
        ishape = (*ctx.lead, meta.K)
        dx = torch.empty(ishape, dtype=meta.dtype, device=dev)
        dxt = [torch.empty(ishape, dtype=meta.dtype, device=dev) for _ in range(nx)]
        has_s = meta.r_s > 0 and (dy_s is not None or (meta.mode == 1 and any(g is not None for g in dy_t)))
        # (a factor that takes no gradient -- the identity side of a rank-aware update, a frozen factor -- is not reduced at all: the
        # library skips the problems whose output pointer is null)
        nA, nB = 10 + nx, 10 + nx + T
        # trainable scales: segment o needs d scale_o = <dB_o, B_o> / scale_o, so dB_o is formed whenever the SCALE needs a gradient, even
        # where B itself is frozen (B then gets None)
        nS = nB + T
        if ctx.has_scale_s or meta.n_scale_t:
            sg_need = [ctx.has_scale_s and need[9] and has_s] + [t < meta.n_scale_t and need[nS + t] and dy_t[t] is not None
                                                                 for t in range(T)]
        else:
            sg_need = (False,) * (1 + T)
        dA_s = torch.empty((meta.r_s, meta.K), dtype=torch.float32, device=dev) if (has_s and need[7]) else None
        dB_s = torch.empty((meta.N, meta.r_s), dtype=torch.float32, device=dev) if (has_s and (need[8] or sg_need[0])) else None
        dA_t = [torch.empty((meta.r_t[t], meta.K), dtype=torch.float32, device=dev) if (dy_t[t] is not None and need[nA + t]) else None
                for t in range(T)]
        dB_t = [torch.empty((meta.N, meta.r_t[t]), dtype=torch.float32, device=dev)
                if (dy_t[t] is not None and (need[nB + t] or sg_need[1 + t])) else None for t in range(T)]
        d_sc = sg_scratch = None
        if any(sg_need):
            d_sc = torch.empty(1 + T, dtype=torch.float32, device=dev)
            sg_scratch = torch.empty(_scale_grad_bytes(), dtype=torch.uint8, device=dev)
            _, B_s_c, _, B_t_c = ctx.keep
            sg_dB = [g if w else None for g, w in zip([dB_s, *dB_t], sg_need)]
            sg_args = (L.ptr_array9(sg_dB), L.ptr_array9([B_s_c, *B_t_c]), L.ptr_array9(meta.scale_dev), 1 + T, L.ptr(d_sc),
                       L.ptr(sg_scratch), sg_scratch.numel())
        if nx:  # a task input whose output got no gradient still needs a defined (zero) gradient
            for t in range(T):
                if dy_t[t] is None:
                    dxt[t].zero_()
        # `linear.bias` trains (mark_only_lora_as_trainable bias='all', reference lora.py:606-624; or FREEZE_PRETRAINED False): every output
        # adds the same x W^T + b, so db is the column sum of the output gradients in hand -- one mtlora_linear_bias_grad over the 1 + T
        # sources, queued with the factor gradients.  A shape the entry refuses (N off the 16-byte vector grid) keeps the ATen form below
        db = db_scratch = None
        db_bytes = -1
        if need[6]:
            db_bytes = _size_query("bias_grad", lib.mtlora_linear_bias_grad_scratch_bytes, d)
        if db_bytes >= 0:
            db = torch.empty(meta.N, dtype=torch.float32, device=dev)
            db_scratch = torch.empty(db_bytes, dtype=torch.uint8, device=dev)
        db_cast = db is not None and ctx.bias_param.dtype != torch.float32  # (the cast reads db on THIS stream)
        # `linear.weight` trains (MODEL.MTLORA.FREEZE_PRETRAINED False, reference main.py:254-262): dW = (sum of the output gradients)^T x
        # with x the shared input the dense product read (x2: un-dropped, gelu(gate) behind a GELU gate) -- one
        # mtlora_linear_weight_grad over the same sources, no (M, N) sum, queued with the factor gradients as well
        dWn = dw_scratch = None
        dw_bytes = -1
        if need[5]:
            dw_bytes = _size_query("weight_grad", lib.mtlora_linear_weight_grad_scratch_bytes, d)
        if dw_bytes >= 0:
            dWn = torch.empty((meta.N, meta.K), dtype=torch.float32, device=dev)
            dw_scratch = torch.empty(dw_bytes, dtype=torch.uint8, device=dev)
        dw_cast = dWn is not None and ctx.weight_param.dtype != torch.float32

        def launch(phase, stream_ptr):
            d.bwd_phase = phase
            if gates:  # the inputs were gelu(gate): the dX epilogue also applies gelu'(gate) (GELU backward fused)
                st = lib.mtlora_linear_bwd_gelu(ctypes.byref(d), L.ptr(x2), L.ptr_array(xt2), L.ptr(Wt_c), L.ptr(dy_s),
                                                L.ptr_array(dy_t), L.ptr(ctxbuf), ctxbuf.numel(), L.ptr(dx), L.ptr_array(dxt),
                                                L.ptr(dA_s), L.ptr(dB_s), L.ptr_array(dA_t), L.ptr_array(dB_t), L.ptr(scratch),
                                                scratch_bytes, L.ptr(gates[0]), L.ptr_array(gates[1:]), stream_ptr)
                L.check(st, "mtlora_linear_bwd_gelu")
            else:
                st = lib.mtlora_linear_bwd(ctypes.byref(d), L.ptr(x2), L.ptr_array(xt2), L.ptr(Wt_c), L.ptr(dy_s),
                                           L.ptr_array(dy_t), L.ptr(ctxbuf), ctxbuf.numel(), L.ptr(dx), L.ptr_array(dxt),
                                           L.ptr(dA_s), L.ptr(dB_s), L.ptr_array(dA_t), L.ptr_array(dB_t), L.ptr(scratch),
                                           scratch_bytes, stream_ptr)
                L.check(st, "mtlora_linear_bwd")
            if d_sc is not None and phase != 1:  # the scale gradients: queued behind the factor gradients, on their stream
                L.check(lib.mtlora_linear_scale_grad(ctypes.byref(d), *sg_args, stream_ptr), "mtlora_linear_scale_grad")
            if db is not None and phase != 1:
                L.check(lib.mtlora_linear_bias_grad(ctypes.byref(d), L.ptr(dy_s), L.ptr_array(dy_t), L.ptr(db), L.ptr(db_scratch), db_bytes,
                                                    stream_ptr), "mtlora_linear_bias_grad")
            if dWn is not None and phase != 1:
                L.check(lib.mtlora_linear_weight_grad(ctypes.byref(d), L.ptr(x2), L.ptr(dy_s), L.ptr_array(dy_t), L.ptr(dWn),
                                                      L.ptr(dw_scratch), dw_bytes, stream_ptr), "mtlora_linear_weight_grad")

        fgrads = [t for t in [dA_s, dB_s, *dA_t, *dB_t, d_sc, sg_scratch, db, db_scratch, dWn, dw_scratch] if t is not None]
        side_params = ctx.factor_params
        if db is not None:
            side_params += (ctx.bias_param,)
        if dWn is not None:
            side_params += (ctx.weight_param,)
        _run_factor_phases(side_params, fgrads, M, dev, not (db_cast or dw_cast), launch,
                           lambda: [x2, ctxbuf, scratch, *xt2, *fgrads] + [g for g in g2 if g is not None])
        dW = dbias = None
        if db is not None:
            dbias = db.to(ctx.bias_param.dtype) if db_cast else db
        if dWn is not None:
            dW = dWn.to(ctx.weight_param.dtype) if dw_cast else dWn
        if (need[5] and dWn is None) or (need[6] and db is None):
            # pretrained weight and / or bias left trainable (MTLORA.FREEZE_PRETRAINED False; mark_only_lora_as_trainable
            # bias='all' trains `linear.bias` with W frozen, reference lora.py:606-617): dense gradients outside the frozen-W
            # hot path.  Every output adds the same base  x W^T + b, so both see G = sum of the output gradients.
            G = None
            for g in g2:
                if g is not None:
                    G = g.reshape(M, meta.N).float() if G is None else G + g.reshape(M, meta.N).float()
            if G is not None:
                if need[5] and dWn is None:
                    dW = G.t() @ x2.reshape(M, meta.K).float()
                if need[6] and db is None:
                    dbias = G.sum(0)
        dxo = dx if ctx.in_dtypes[0] == meta.dtype else dx.to(ctx.in_dtypes[0])
        dxto = [dxt[t] if ctx.in_dtypes[1 + t] == meta.dtype else dxt[t].to(ctx.in_dtypes[1 + t]) for t in range(nx)]
        d_ss = d_sc[0:1] if (d_sc is not None and sg_need[0]) else None
        d_st = [d_sc[1 + t:2 + t] if (d_sc is not None and sg_need[1 + t]) else None for t in range(meta.n_scale_t)]
        if not need[8]:
            dB_s = None  # (formed for the scale's gradient only)
        dB_t = [g if need[nB + t] else None for t, g in enumerate(dB_t)]
        return (None, dxo, None, None, None, dW, dbias, dA_s, dB_s, d_ss, *dxto, *dA_t, *dB_t, *d_st, *([None] * meta.n_gate))


# ----------------------------------------------------------------------------------------------
# Task-enabled Mlp with IMPLICIT task hidden tensors (csrc/hid.hip, ABI v8)
# ----------------------------------------------------------------------------------------------
_MLP_HID = os.environ.get("MTLORA_MLP_HID", "1") != "0"


def mlp_hid_enabled() -> bool:
    return _MLP_HID


def set_mlp_hid(on: bool) -> bool:
    """switch the implicit-task-hiddens path of the task-enabled Mlp on / off (tests compare the two paths); returns the old value"""
    global _MLP_HID
    old, _MLP_HID = _MLP_HID, bool(on)
    return old


def mlp_hid_supported(meta1: "LinearMeta", meta2: "LinearMeta", M: int) -> bool:
    return bool(_size_query("hid_ok", L.lib().mtlora_mlp_hid_supported, meta1.desc(M), meta2.desc(M)))


def _ensure_packed(meta: "LinearMeta", A_s, B_s, A_t, B_t, device) -> None:
    """the k_hid kernels read the layers' packed factors: a layer without a current FactorPacker buffer packs into a per-call one"""
    if meta.packed is not None:
        return
    buf = torch.empty(packed_bytes(meta), dtype=torch.uint8, device=device)
    d = meta.desc(1)
    d.packed = 0
    st = L.lib().mtlora_linear_pack(ctypes.byref(d), L.ptr(A_s), L.ptr(B_s), L.ptr_array(A_t), L.ptr_array(B_t), L.ptr(buf), buf.numel(),
                                    L.stream_ptr())
    L.check(st, "mtlora_linear_pack")
    meta.packed = buf


class MlpHidFn(torch.autograd.Function):
    """(y_s, y_t[0..T-1]) = fc2(gelu(fc1(x, x_t)), gelu(fc1 task outputs)) of a task-enabled Mlp (swin_transformer_mtlora.py:57-78 of the
    reference with both layers MTLoRALinear called with x_tasks, lora.py:262-266) WITHOUT the 3 T hidden-width task tensors of the
    per-layer path: h_t = h_base + P1_t B1_t^T only enters fc2 through P2_t = s_t gelu(h_t) A2_t^T, and its gradient only feeds
    G, Q1_t and two rank-r_t factor gradients (csrc/hid.hip).  Same parameters, same results up to rounding (the implicit tensors stay
    in fp32 registers instead of being rounded to the compute dtype).

    args: meta1, meta2, x, W1c, W1t, b1, W2c, W2t, b2, A1_s, B1_s, A2_s, B2_s, *x_t(T), *A1_t(T), *B1_t(T), *A2_t(T), *B2_t(T)"""

    NFIX = 13

    @staticmethod
    def forward(ctx, meta1: LinearMeta, meta2: LinearMeta, x, W1c, W1t, b1, W2c, W2t, b2, A1_s, B1_s, A2_s, B2_s, *rest):
        ctx.set_materialize_grads(False)
        T = meta1.T
        x_t = list(rest[:T])
        A1_t, B1_t, A2_t, B2_t = (list(rest[T * k:T * (k + 1)]) for k in range(1, 5))
        L.require_gpu(x, W1c, W2c, *x_t)
        lead = x.shape[:-1]
        x2 = _flat(x, meta1.dtype)
        xt2 = [_flat(t, meta1.dtype) for t in x_t]
        M = x2.numel() // meta1.K
        if x2.shape[-1] != meta1.K or any(t.shape != x2.shape for t in xt2):
            raise RuntimeError(f"mtlora_amd: Mlp input of shape {tuple(x.shape)} for in_features = {meta1.K}")
        dev, dt, H = x.device, meta1.dtype, meta1.N
        f1 = (_f32c(A1_s), _f32c(B1_s), [_f32c(a) for a in A1_t], [_f32c(b) for b in B1_t])
        f2 = (_f32c(A2_s), _f32c(B2_s), [_f32c(a) for a in A2_t], [_f32c(b) for b in B2_t])
        _ensure_packed(meta1, *f1, dev)
        _ensure_packed(meta2, *f2, dev)
        lib = L.lib()
        d1, d2 = meta1.desc(M), meta2.desc(M)
        cb1 = _size_query("ctx", lib.mtlora_linear_ctx_bytes, d1)
        cb2 = _size_query("ctx", lib.mtlora_linear_ctx_bytes, d2)
        ctx1 = _scratch(cb1, dev, "Mlp shape (M, K, hidden, N)", M, meta1.K, H, meta2.N)
        ctx2 = _scratch(cb2, dev, "Mlp shape (M, K, hidden, N)", M, meta1.K, H, meta2.N)
        hshape = (*lead, H)
        h_s = torch.empty(hshape, dtype=dt, device=dev)
        a_s = torch.empty(hshape, dtype=dt, device=dev)
        h_base = torch.empty(hshape, dtype=dt, device=dev)
        # fc1: shared output (+ its GELU) and the bare pretrained product; P1 for every segment
        d1.hid, d1.hid_ptr = L.HID_FWD_BASE, h_base.data_ptr()
        st = lib.mtlora_linear_fwd_gelu(ctypes.byref(d1), L.ptr(x2), L.ptr_array(xt2), L.ptr(W1c), L.ptr(b1), L.ptr(f1[0]), L.ptr(f1[1]),
                                        L.ptr_array(f1[2]), L.ptr_array(f1[3]), L.ptr(h_s), L.ptr_array(None), L.ptr(a_s),
                                        L.ptr_array(None), L.ptr(ctx1), cb1, L.stream_ptr())
        L.check(st, "mtlora_linear_fwd_gelu (fc1, implicit task hiddens)")
        d1.hid, d1.hid_ptr = 0, 0
        # the task columns of fc2's P straight from h_base and P1
        fb = _size_query("hid_fwd", lib.mtlora_mlp_hid_fwd_scratch_bytes, d1, d2)
        fscr = _scratch(fb, dev, "Mlp shape (M, K, hidden, N) for implicit task hiddens", M, meta1.K, H, meta2.N)
        st = lib.mtlora_mlp_hid_proj(ctypes.byref(d1), ctypes.byref(d2), L.ptr(h_base), L.ptr(ctx1), L.ptr(ctx2), L.ptr(fscr), fb,
                                     L.stream_ptr())
        L.check(st, "mtlora_mlp_hid_proj")
        oshape = (*lead, meta2.N)
        ys = torch.empty(oshape, dtype=dt, device=dev)
        yt = [torch.empty(oshape, dtype=dt, device=dev) for _ in range(T)]
        d2.hid = L.HID_P_GIVEN
        st = lib.mtlora_linear_fwd(ctypes.byref(d2), L.ptr(a_s), L.ptr_array(None), L.ptr(W2c), L.ptr(b2), L.ptr(f2[0]), L.ptr(f2[1]),
                                   L.ptr_array(f2[2]), L.ptr_array(f2[3]), L.ptr(ys), L.ptr_array(yt), L.ptr(ctx2), cb2, L.stream_ptr())
        L.check(st, "mtlora_linear_fwd (fc2, implicit task hiddens)")
        ctx.meta1, ctx.meta2, ctx.lead, ctx.M = meta1, meta2, lead, M
        ctx.in_dtypes = [x.dtype] + [t.dtype for t in x_t]
        ctx.save_for_backward(x2, W1t, W2t, ctx1, ctx2, h_s, a_s, h_base, *xt2)
        ctx.factor_params = (A1_s, B1_s, *A1_t, *B1_t, A2_s, B2_s, *A2_t, *B2_t)
        return (ys, *yt)

    @staticmethod
    def backward(ctx, *grads):
        meta1, meta2 = ctx.meta1, ctx.meta2
        T, NF = meta1.T, MlpHidFn.NFIX
        n_in = NF + 5 * T
        if all(g is None for g in grads):
            return (None,) * n_in
        x2, W1t, W2t, ctx1, ctx2, h_s, a_s, h_base, *xt2 = ctx.saved_tensors
        M, dev, dt, H = ctx.M, x2.device, meta1.dtype, meta1.N
        g2 = [None if g is None else _flat(g, dt) for g in grads]
        dy_s, dy_t = g2[0], g2[1:1 + T]
        need = ctx.needs_input_grad
        lib = L.lib()
        d1, d2 = meta1.desc(M), meta2.desc(M)
        sb1 = _size_query("bwd", lib.mtlora_linear_bwd_scratch_bytes, d1)
        sb2 = _size_query("bwd", lib.mtlora_linear_bwd_scratch_bytes, d2)
        pb = _size_query("hid_bwd", lib.mtlora_mlp_hid_bwd_scratch_bytes, d1, d2)
        scratch1 = _scratch(sb1, dev, "Mlp backward shape (M, K, hidden)", M, meta1.K, H)
        scratch2 = _scratch(sb2, dev, "Mlp backward shape (M, hidden, N)", M, H, meta2.N)
        part = _scratch(pb, dev, "Mlp backward shape (M, K, hidden, N) for implicit task hiddens", M, meta1.K, H, meta2.N)
        f32 = torch.float32
        hshape, ishape = (*ctx.lead, H), (*ctx.lead, meta1.K)
        dh_s = torch.empty(hshape, dtype=dt, device=dev)
        G = torch.empty(hshape, dtype=dt, device=dev)
        dx = torch.empty(ishape, dtype=dt, device=dev)
        dxt = [torch.empty(ishape, dtype=dt, device=dev) for _ in range(T)]
        # argument positions: A1_s 9, B1_s 10, A2_s 11, B2_s 12, x_t NF.., A1_t NF+T.., B1_t NF+2T.., A2_t NF+3T.., B2_t NF+4T..
        has_s2 = meta2.r_s > 0 and dy_s is not None
        has_s1 = meta1.r_s > 0
        any_t = [dy_t[t] is not None for t in range(T)]
        dA1_s = torch.empty((meta1.r_s, meta1.K), dtype=f32, device=dev) if (has_s1 and need[9]) else None
        dB1_s = torch.empty((H, meta1.r_s), dtype=f32, device=dev) if (has_s1 and need[10]) else None
        dA2_s = torch.empty((meta2.r_s, H), dtype=f32, device=dev) if (has_s2 and need[11]) else None
        dB2_s = torch.empty((meta2.N, meta2.r_s), dtype=f32, device=dev) if (has_s2 and need[12]) else None
        mk = lambda shape, pos, t: torch.empty(shape, dtype=f32, device=dev) if (any_t[t] and need[pos + t]) else None
        dA1_t = [mk((meta1.r_t[t], meta1.K), NF + T, t) for t in range(T)]
        dB1_t = [mk((H, meta1.r_t[t]), NF + 2 * T, t) for t in range(T)]
        dA2_t = [mk((meta2.r_t[t], H), NF + 3 * T, t) for t in range(T)]
        dB2_t = [mk((meta2.N, meta2.r_t[t]), NF + 4 * T, t) for t in range(T)]

        def fc2(phase, stream_ptr):  # dh_s (through gelu'(h_s)), Q2 [phase 1]; dA2_s, dB2_s, dB2_t [phase 2]
            d2.bwd_phase = phase
            st = lib.mtlora_linear_bwd_gelu(ctypes.byref(d2), L.ptr(a_s), L.ptr_array(None), L.ptr(W2t), L.ptr(dy_s), L.ptr_array(dy_t),
                                            L.ptr(ctx2), ctx2.numel(), L.ptr(dh_s), L.ptr_array(None), L.ptr(dA2_s), L.ptr(dB2_s),
                                            L.ptr_array(None), L.ptr_array(dB2_t), L.ptr(scratch2), sb2, L.ptr(h_s), L.ptr_array(None),
                                            stream_ptr)
            L.check(st, "mtlora_linear_bwd_gelu (fc2, implicit task hiddens)")

        def hid(stream_ptr):  # G = dh_s + sum_t dH_t, Q1 task columns, dB1_t, dA2_t
            st = lib.mtlora_mlp_hid_bwd(ctypes.byref(d1), ctypes.byref(d2), L.ptr(h_base), L.ptr(dh_s), L.ptr(ctx1), L.ptr(ctx2),
                                        L.ptr(scratch2), L.ptr(scratch1), L.ptr(G), L.ptr_array(dB1_t), L.ptr_array(dA2_t), L.ptr(part), pb,
                                        stream_ptr)
            L.check(st, "mtlora_mlp_hid_bwd")

        def fc1(phase, stream_ptr):  # dx, dx_t [phase 1]; dA1_s, dB1_s, dA1_t [phase 2]
            d1.bwd_phase = phase
            d1.hid, d1.hid_ptr = L.HID_Q_GIVEN, G.data_ptr()
            st = lib.mtlora_linear_bwd(ctypes.byref(d1), L.ptr(x2), L.ptr_array(xt2), L.ptr(W1t), L.ptr(dh_s), L.ptr_array(None),
                                       L.ptr(ctx1), ctx1.numel(), L.ptr(dx), L.ptr_array(dxt), L.ptr(dA1_s), L.ptr(dB1_s),
                                       L.ptr_array(dA1_t), L.ptr_array(None), L.ptr(scratch1), sb1, stream_ptr)
            L.check(st, "mtlora_linear_bwd (fc1, implicit task hiddens)")

        def run(phase, stream_ptr):  # fc2(1), hid, fc1(1) | fc2(2), fc1(2)
            if phase != 2:
                fc2(1, stream_ptr)
                hid(stream_ptr)
                fc1(1, stream_ptr)
            if phase != 1:
                fc2(2, stream_ptr)
                fc1(2, stream_ptr)

        fgrads = [t for t in [dA1_s, dB1_s, dA2_s, dB2_s, *dA1_t, *dB1_t, *dA2_t, *dB2_t] if t is not None]
        _run_factor_phases(ctx.factor_params, fgrads, M, dev, True, run,
                           lambda: [x2, ctx1, ctx2, a_s, dh_s, scratch1, scratch2, *xt2, *fgrads] + [g for g in g2 if g is not None])
        dxo = dx if ctx.in_dtypes[0] == dt else dx.to(ctx.in_dtypes[0])
        dxto = [dxt[t] if ctx.in_dtypes[1 + t] == dt else dxt[t].to(ctx.in_dtypes[1 + t]) for t in range(T)]
        return (None, None, dxo, None, None, None, None, None, None, dA1_s, dB1_s, dA2_s, dB2_s, *dxto, *dA1_t, *dB1_t, *dA2_t, *dB2_t)


class GeluDeferredGradFn(torch.autograd.Function):
    """a = gelu(h) (exact erf form) whose backward is the IDENTITY: the consumer is an MTLoRALinear called with
    ``gelu_gate=h``, whose dX kernel multiplies by gelu'(h) itself (``mtlora_linear_bwd_gelu``) -- the standalone GELU
    backward pass (read dA, read h, write dH) disappears.  Only ``Mlp.forward`` pairs the two."""

    @staticmethod
    def forward(ctx, h):
        return torch.nn.functional.gelu(h)

    @staticmethod
    def backward(ctx, g):
        return g


# ----------------------------------------------------------------------------------------------
# window attention core
# ----------------------------------------------------------------------------------------------
@dataclass
class AttnMeta:
    B: int
    H: int
    W: int
    window_size: int
    shift: int
    num_heads: int
    head_dim: int
    image_layout: bool
    scale: float
    mask_value: float = -100.0

    def desc(self, dtype: torch.dtype) -> L.AttnDesc:
        d = L.AttnDesc()
        d.B, d.H, d.W = self.B, self.H, self.W
        d.window_size, d.shift = self.window_size, self.shift
        d.num_heads, d.head_dim = self.num_heads, self.head_dim
        d.image_layout = 1 if self.image_layout else 0
        d.dtype = L._DT[dtype]
        d.scale = self.scale
        d.mask_value = self.mask_value
        return d


class WindowAttentionFn(torch.autograd.Function):
    """out = softmax(scale * q k^T + bias[h] + mask[w]) v per (window, head)  (swin_transformer_mtlora.py:194-220).
    qkv: (..., 3C) [3][nH][hd]; bias: (nH, N, N) fp32 dense.  The shift mask is either ``mask_ids`` (nW, N) int32
    region ids (fast path: mask(i,j) = ids differ ? meta.mask_value : 0) or a general dense ``mask`` (nW, N, N).
    Optional ``p, seed``: attention dropout on the softmax output (reference :216), generated inside the kernels from ``seed`` (plus
    the device seed-offset word of :func:`set_seed_offset`, as the linear layers); the backward regenerates the same bits."""

    @staticmethod
    def forward(ctx, meta: AttnMeta, qkv, bias, mask, mask_ids, *drop):
        p, seed = (float(drop[0]), int(drop[1])) if drop else (0.0, 0)
        L.require_gpu(qkv, bias, mask, mask_ids)
        dt = qkv.dtype
        if dt not in _HOT_DTYPES:
            raise RuntimeError(f"mtlora_amd: window attention supports fp32 / bf16 / fp16, got {dt}")
        qkv_c = qkv.contiguous()
        bias_c = _f32_param(bias)
        if mask_ids is not None:
            mask_ids = mask_ids.to(torch.int32).contiguous()
            mask = None
        elif mask is not None:
            mask = mask.float().contiguous()
        C = meta.num_heads * meta.head_dim
        out = torch.empty(qkv_c.shape[:-1] + (C,), dtype=dt, device=qkv.device)
        d = meta.desc(dt)
        if p > 0.0:
            dr = L.AttnDropout()
            dr.p, dr.seed, dr.seed_offset = p, seed, (0 if _seed_offset is None else _seed_offset.data_ptr())
            st = L.lib().mtlora_window_attn_drop_fwd(ctypes.byref(d), ctypes.byref(dr), L.ptr(qkv_c), L.ptr(bias_c), L.ptr(mask),
                                                     L.ptr(mask_ids), L.ptr(out), L.stream_ptr())
            L.check(st, "mtlora_window_attn_drop_fwd")
        else:
            dr = None
            st = L.lib().mtlora_window_attn_fwd(ctypes.byref(d), L.ptr(qkv_c), L.ptr(bias_c), L.ptr(mask), L.ptr(mask_ids),
                                                L.ptr(out), L.stream_ptr())
            L.check(st, "mtlora_window_attn_fwd")
        ctx.meta, ctx.drop, ctx.n_drop = meta, dr, len(drop)
        ctx.save_for_backward(qkv_c, bias_c, mask, mask_ids)
        return out

    @staticmethod
    def backward(ctx, dout):
        meta: AttnMeta = ctx.meta
        qkv, bias, mask, mask_ids = ctx.saved_tensors
        dout = dout.to(qkv.dtype).contiguous()
        d = meta.desc(qkv.dtype)
        lib = L.lib()
        sb = lib.mtlora_window_attn_bwd_scratch_bytes(ctypes.byref(d))
        scratch = _scratch(sb, qkv.device, "window attention geometry (B, H, W, window)", meta.B, meta.H, meta.W, meta.window_size)
        dqkv = torch.empty_like(qkv)
        dbias = torch.empty_like(bias)
        if ctx.drop is not None:
            st = lib.mtlora_window_attn_drop_bwd(ctypes.byref(d), ctypes.byref(ctx.drop), L.ptr(qkv), L.ptr(bias), L.ptr(mask),
                                                 L.ptr(mask_ids), L.ptr(dout), L.ptr(dqkv), L.ptr(dbias), L.ptr(scratch), sb,
                                                 L.stream_ptr())
            L.check(st, "mtlora_window_attn_drop_bwd")
        else:
            st = lib.mtlora_window_attn_bwd(ctypes.byref(d), L.ptr(qkv), L.ptr(bias), L.ptr(mask), L.ptr(mask_ids),
                                            L.ptr(dout), L.ptr(dqkv), L.ptr(dbias), L.ptr(scratch), sb, L.stream_ptr())
            L.check(st, "mtlora_window_attn_bwd")
        return (None, dqkv, dbias, None, None) + (None,) * ctx.n_drop


# ----------------------------------------------------------------------------------------------
# window process (kernels/window_process/window_process.py)
# ----------------------------------------------------------------------------------------------
def _wp(fn_name: str, src: torch.Tensor, out_shape, B, H, W, C, shift_size, window_size) -> torch.Tensor:
    L.require_gpu(src)
    if not src.is_contiguous():
        raise RuntimeError("input must be contiguous")  # CHECK_CONTIGUOUS, swin_window_process.cpp:65
    if src.numel() != B * H * W * C:
        raise RuntimeError(f"mtlora_amd: {fn_name}: tensor has {src.numel()} elements, expected B*H*W*C={B * H * W * C}")
    out = torch.empty(out_shape, dtype=src.dtype, device=src.device)
    st = getattr(L.lib(), fn_name)(L.ptr(src), L.ptr(out), B, H, W, C, shift_size, window_size,
                                   L.dtype_code(src, allow_f16=True), L.stream_ptr())
    L.check(st, fn_name)
    return out


def roll_and_window_partition_forward(input, B, H, W, C, shift_size, window_size):
    n = B * (H // window_size) * (W // window_size)
    return _wp("mtlora_roll_and_window_partition_forward", input, (n, window_size, window_size, C), B, H, W, C,
               shift_size, window_size)


def roll_and_window_partition_backward(grad_in, B, H, W, C, shift_size, window_size):
    return _wp("mtlora_roll_and_window_partition_backward", grad_in, (B, H, W, C), B, H, W, C, shift_size, window_size)


def window_merge_and_roll_forward(input, B, H, W, C, shift_size, window_size):
    return _wp("mtlora_window_merge_and_roll_forward", input, (B, H, W, C), B, H, W, C, shift_size, window_size)


def window_merge_and_roll_backward(grad_in, B, H, W, C, shift_size, window_size):
    n = B * (H // window_size) * (W // window_size)
    return _wp("mtlora_window_merge_and_roll_backward", grad_in, (n, window_size, window_size, C), B, H, W, C,
               shift_size, window_size)


# ----------------------------------------------------------------------------------------------
# LayerNorm (block glue): reads x once, writes y directly in the dtype the next linear consumes
# ----------------------------------------------------------------------------------------------
def _ln_module_ok(mod: torch.nn.Module, last_dim_only: bool = False) -> bool:
    """an affine ``nn.LayerNorm`` with a bias, nothing derived from it (``last_dim_only``: normalised over one dim; the merge
    forms do not ask)"""
    return (type(mod) is torch.nn.LayerNorm and mod.elementwise_affine and mod.bias is not None
            and (not last_dim_only or len(mod.normalized_shape) == 1))


def _ln_width_ok(x: torch.Tensor, multiple: int, width: int, cap=(2048, 4096)) -> bool:
    """x on the GPU in a kernel dtype, its last dim a multiple of ``multiple``, and the normalised ``width`` within
    ``cap`` = (fp32 limit, 16-bit limit)"""
    return (x.is_cuda and x.dtype in _GLUE_DTYPES and x.shape[-1] % multiple == 0
            and width <= cap[0 if x.dtype == torch.float32 else 1])


def _ln_vec(x: torch.Tensor) -> int:
    """elements per 16-byte vector: what the token width of the merge forms must be a multiple of"""
    return 4 if x.dtype == torch.float32 else 8


def _ln_affine(weight, bias):
    """(gamma, beta) as the kernels read them: fp32, contiguous"""
    return _f32_param(weight), _f32_param(bias)


def _kernel_dtype(dt: torch.dtype) -> torch.dtype:
    """a gradient's own dtype if the glue kernels read it, else fp32"""
    return dt if dt in _GLUE_DTYPES else torch.float32


def _canon_grad(g: Optional[torch.Tensor], shape, dtype: torch.dtype) -> Optional[torch.Tensor]:
    """an incoming gradient as a kernel reads it: of ``shape``, contiguous, in the ``dtype`` the caller names (None stays None)"""
    if g is None:
        return None
    g = g.reshape(shape)
    return (g if g.dtype == dtype else g.to(dtype)).contiguous()


def _droppath_scale_for(n: int, B: int, drop_prob: float, training: bool, device) -> Optional[torch.Tensor]:
    """the (n, B) DropPath factors of a residual (``droppath_scale``), or None when DropPath is off"""
    if training and drop_prob > 0.0:
        return droppath_scale(n, B, 1.0 - drop_prob, device)
    return None


def _merge_ok(mod: torch.nn.Module, x: torch.Tensor, H: int, W: int) -> bool:
    """may the PatchMerging forms gather the 2x2 neighbourhoods of the (B, H*W, C) token tensor ``x`` for ``mod``?"""
    _, Lt, C = x.shape
    return (_ln_module_ok(mod) and _ln_width_ok(x, multiple=_ln_vec(x), width=4 * C) and Lt == H * W and H % 2 == 0 and W % 2 == 0)


def _streams_ok(xs) -> bool:
    """2 .. MAX_TASKS + 1 device tensors of one dtype and shape"""
    return (2 <= len(xs) <= L.MAX_TASKS + 1 and all(x.is_cuda and x.dtype == xs[0].dtype and x.shape == xs[0].shape for x in xs))


def _ln_row_stats(M: int, device):
    return torch.empty(M, dtype=torch.float32, device=device), torch.empty(M, dtype=torch.float32, device=device)


def _ln_stream_stats(n: int, M: int, device=None, stats=None):
    """(stats, means, rstds): one (2n, M) fp32 tensor (saved for the backward, which passes it back in) and its per-stream rows"""
    if stats is None:
        stats = torch.empty((2 * n, M), dtype=torch.float32, device=device)
    return stats, [stats[k] for k in range(n)], [stats[n + k] for k in range(n)]


def _ln_bwd_buffers(M: int, C: int, x: torch.Tensor, n=None):
    """(scratch, scratch bytes, dgamma, dbeta) of a backward call; ``n``: streams of the multi_x forms (their partials are per
    stream)"""
    lib, code = L.lib(), L.dtype_code(x)
    sb = (lib.mtlora_layernorm_bwd_scratch_bytes(M, C, code) if n is None
          else lib.mtlora_layernorm_multi_bwd_scratch_bytes(n, M, C, code))
    scratch = _scratch(sb, x.device, "LayerNorm backward shape (M, C)", M, C)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    return scratch, sb, dg, db


def _ln_forward(ctx, x, weight, bias, eps, out_dtype, merge=None):
    """merge=(H, W): x is a (B, H*W, C) token tensor and the normalised rows are its 2x2 neighbourhoods (PatchMerging):
    output (B, H*W/4, 4C), gathered by the kernel."""
    L.require_gpu(x, weight, bias)
    if merge is None:
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        M, mh, mw = x2.shape[0], 0, 0
        out_shape = x.shape
    else:
        mh, mw = merge
        B, Lt, Ct = x.shape
        C, M = 4 * Ct, B * Lt // 4
        x2 = x.contiguous()
        out_shape = (B, Lt // 4, C)
    w, b = _ln_affine(weight, bias)
    y = torch.empty((M, C), dtype=out_dtype, device=x.device)
    mean, rstd = _ln_row_stats(M, x.device)
    st = L.lib().mtlora_layernorm_fwd(L.ptr(x2), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(mean), L.ptr(rstd), M, C,
                                      float(eps), L.dtype_code(x2), L.dtype_code(y), mh, mw, L.stream_ptr())
    L.check(st, "mtlora_layernorm_fwd")
    ctx.save_for_backward(x2, w, mean, rstd)
    ctx.shape, ctx.merge, ctx.MC = x.shape, (mh, mw), (M, C)
    return y.reshape(out_shape)


def _ln_backward(ctx, dy, addend=None):
    """dx (+ addend), dgamma, dbeta"""
    x2, w, mean, rstd = ctx.saved_tensors
    M, C = ctx.MC
    mh, mw = ctx.merge
    dy2 = _canon_grad(dy, (M, C), _kernel_dtype(dy.dtype))
    add2 = _canon_grad(addend, x2.shape, x2.dtype)
    scratch, sb, dg, db = _ln_bwd_buffers(M, C, x2)
    dx = torch.empty_like(x2)
    st = L.lib().mtlora_layernorm_bwd(L.ptr(dy2), L.ptr(x2), L.ptr(w), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dg),
                                  L.ptr(db), M, C, L.dtype_code(x2), L.dtype_code(dy2), L.ptr(scratch), sb, L.ptr(add2),
                                  mh, mw, L.stream_ptr())
    L.check(st, "mtlora_layernorm_bwd")
    return dx.reshape(ctx.shape), dg, db


class LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x) (``merge``: of the 2x2 neighbourhoods, see ``_ln_forward``).  ``fork``: (x_skip, y) = (x, LayerNorm(x)) --
    the block input feeds the LayerNorm AND the residual connection.  Routing both uses through one node lets the backward form
    d x = g_skip + LN-backward(g_y)  inside the LayerNorm kernel (``dx_addend``) instead of autograd's separate full-size
    gradient add (one per stream per half block)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, out_dtype: torch.dtype, merge=None, fork: bool = False):
        y = _ln_forward(ctx, x, weight, bias, eps, out_dtype, merge)
        ctx.fork = fork
        return (x.view_as(x), y) if fork else y

    @staticmethod
    def backward(ctx, *grads):  # (g_y), or (g_skip, g_y) of the fork form: both materialised
        dx, dg, db = _ln_backward(ctx, grads[-1], grads[0] if ctx.fork else None)
        return dx, dg, db, None, None, None, None


class ResidualLayerNormFn(torch.autograd.Function):
    """(x_new, y) = (shortcut + scale[sample] * branch, LayerNorm(x_new)) as ONE kernel; x_new is the next skip path
    (a fork, as ``LayerNormFn(fork=True)``), y feeds the following linear.  Backward: d_shortcut = g_x_new +
    LN-backward(g_y), d_branch = scale * d_shortcut, both written by the LayerNorm backward kernel
    (``mtlora_residual_layernorm_fwd/bwd``).  Replaces ResidualDropPathFn + the LayerNorm fork for a single stream."""

    @staticmethod
    def forward(ctx, shortcut, branch, scale, weight, bias, eps: float, out_dtype: torch.dtype):
        L.require_gpu(shortcut, branch, weight, bias)
        C = shortcut.shape[-1]
        B = shortcut.shape[0]
        s2 = shortcut.reshape(-1, C).contiguous()
        b2 = branch.reshape(-1, C).contiguous()
        M = s2.shape[0]
        w, b = _ln_affine(weight, bias)
        x_new = torch.empty_like(s2)
        y = torch.empty((M, C), dtype=out_dtype, device=s2.device)
        mean, rstd = _ln_row_stats(M, s2.device)
        st = L.lib().mtlora_residual_layernorm_fwd(L.ptr(s2), L.ptr(b2), L.ptr(scale), B, L.ptr(w), L.ptr(b), L.ptr(x_new),
                                                   L.ptr(y), L.ptr(mean), L.ptr(rstd), M, C, float(eps), L.dtype_code(s2),
                                                   L.dtype_code(y), L.stream_ptr())
        L.check(st, "mtlora_residual_layernorm_fwd")
        ctx.save_for_backward(x_new, w, mean, rstd, scale)
        ctx.shape, ctx.MC, ctx.B, ctx.bdtype = shortcut.shape, (M, C), B, branch.dtype
        ctx.set_materialize_grads(False)
        return x_new.view(shortcut.shape), y.view(shortcut.shape)

    @staticmethod
    def backward(ctx, g_skip, gy):
        x_new, w, mean, rstd, scale = ctx.saved_tensors
        M, C = ctx.MC
        if gy is None:  # the normalised output was not used: plain residual backward
            if g_skip is None:
                return (None,) * 7
            g = g_skip.reshape(ctx.B, -1, C)
            db_ = g if scale is None else g * scale.view(-1, 1, 1).to(g.dtype)
            return g_skip, db_.to(ctx.bdtype).reshape(ctx.shape), None, None, None, None, None
        dy2 = _canon_grad(gy, (M, C), ctx.bdtype)
        add2 = _canon_grad(g_skip, (M, C), x_new.dtype)
        scratch, sb, dg, db = _ln_bwd_buffers(M, C, x_new)
        dx = torch.empty_like(x_new)
        dbr = torch.empty((M, C), dtype=ctx.bdtype, device=x_new.device)
        st = L.lib().mtlora_residual_layernorm_bwd(L.ptr(dy2), L.ptr(x_new), L.ptr(w), L.ptr(mean), L.ptr(rstd), L.ptr(dx),
                                               L.ptr(dbr), L.ptr(dg), L.ptr(db), L.ptr(scale), ctx.B, M, C,
                                               L.dtype_code(x_new), L.dtype_code(dy2), L.ptr(scratch), sb, L.ptr(add2),
                                               L.stream_ptr())
        L.check(st, "mtlora_residual_layernorm_bwd")
        return dx.view(ctx.shape), dbr.view(ctx.shape), None, dg, db, None, None


class ResidualLayerNormMultiFn(torch.autograd.Function):
    """Task-enabled block half: ONE shortcut, n branches -> (x_new_0..n-1, y_0..n-1) with x_new_k = shortcut + scale[k] *
    branch_k and y_k = LayerNorm(x_new_k), one kernel; backward one kernel: d_branch_k = scale[k] * dx_k, d_shortcut = sum_k
    dx_k, dx_k = g_x_new_k + LN'(g_y_k) (never stored), dgamma / dbeta over all streams.
    args: scale ((n, B) fp32 or None), weight, bias, eps, out_dtype, n, shortcut, *branches"""

    @staticmethod
    def forward(ctx, scale, weight, bias, eps: float, out_dtype: torch.dtype, n: int, shortcut, *branches):
        L.require_gpu(shortcut, weight, bias, *branches)
        C, B = shortcut.shape[-1], shortcut.shape[0]
        s2 = shortcut.reshape(-1, C).contiguous()
        bs = [b.reshape(-1, C).contiguous() for b in branches]
        M = s2.shape[0]
        w, b = _ln_affine(weight, bias)
        xs = [torch.empty_like(s2) for _ in range(n)]
        ys = [torch.empty((M, C), dtype=out_dtype, device=s2.device) for _ in range(n)]
        stats, means, rstds = _ln_stream_stats(n, M, s2.device)
        st = L.lib().mtlora_residual_layernorm_multi_fwd(n, L.ptr(s2), L.ptr_array9(bs), L.ptr(scale), B, L.ptr(w), L.ptr(b),
                                                         L.ptr_array9(xs), L.ptr_array9(ys), L.ptr_array9(means),
                                                         L.ptr_array9(rstds), M, C, float(eps), L.dtype_code(s2),
                                                         L.dtype_code(ys[0]), L.stream_ptr())
        L.check(st, "mtlora_residual_layernorm_multi_fwd")
        ctx.save_for_backward(w, stats, scale, *xs)
        ctx.shape, ctx.MC, ctx.B, ctx.n, ctx.bdtype = shortcut.shape, (M, C), B, n, branches[0].dtype
        return tuple(x.view(shortcut.shape) for x in xs) + tuple(y.view(shortcut.shape) for y in ys)

    @staticmethod
    def backward(ctx, *grads):
        w, stats, scale, *xs = ctx.saved_tensors
        n, (M, C) = ctx.n, ctx.MC
        g_skip, g_y = grads[:n], grads[n:]
        dev = xs[0].device
        dys = [_canon_grad(g, (M, C), ctx.bdtype) for g in g_y]             # (materialised: zeros if unused)
        adds = [_canon_grad(g, (M, C), xs[0].dtype) for g in g_skip]
        scratch, sb, dg, db = _ln_bwd_buffers(M, C, xs[0])
        dsh = torch.empty_like(xs[0])
        dbr = [torch.empty((M, C), dtype=ctx.bdtype, device=dev) for _ in range(n)]
        _, means, rstds = _ln_stream_stats(n, M, stats=stats)
        st = L.lib().mtlora_residual_layernorm_multi_bwd(n, L.ptr_array9(dys), L.ptr_array9(xs), L.ptr(w), L.ptr_array9(means),
                                                     L.ptr_array9(rstds), L.ptr_array9(adds), L.ptr(dsh), L.ptr_array9(dbr),
                                                     L.ptr(dg), L.ptr(db), L.ptr(scale), ctx.B, M, C, L.dtype_code(xs[0]),
                                                     L.dtype_code(dys[0]), L.ptr(scratch), sb, L.stream_ptr())
        L.check(st, "mtlora_residual_layernorm_multi_bwd")
        return (None, dg, db, None, None, None, dsh.view(ctx.shape), *[d.view(ctx.shape) for d in dbr])


def residual_layer_norm_multi(mod: torch.nn.Module, shortcut: torch.Tensor, branches, drop_prob: float, training: bool, drop=None):
    """([x_new_k], [mod(x_new_k)]) with x_new_k = shortcut + DropPath_k(branches[k]) (an independent per-sample mask per k):
    the fused multi-stream kernels when they apply, else residual_droppath + layer_norm_fork per stream.  ``drop``: a pending
    activation dropout of the branches (``residual_droppath``): the fused residual + LayerNorm forms have no dropout."""
    C, n = shortcut.shape[-1], len(branches)
    if drop is not None:
        forks = [layer_norm_fork(mod, x) for x in residual_droppath(shortcut, list(branches), drop_prob, training, drop)]
        return [f[0] for f in forks], [f[1] for f in forks]
    ok = (_ln_module_ok(mod, last_dim_only=True) and _ln_width_ok(shortcut, multiple=8, width=C, cap=(1024, 1536))
          and shortcut.dim() == 3 and 1 <= n <= L.MAX_TASKS + 1 and all(b.shape == shortcut.shape for b in branches) and torch.is_grad_enabled()
          and (shortcut.requires_grad or any(b.requires_grad for b in branches)))
    if ok:
        out_dtype = glue_dtype(shortcut)
        ok = all(b.dtype == out_dtype for b in branches)
    if not ok:
        r = residual_droppath(shortcut, list(branches), drop_prob, training)
        forks = [layer_norm_fork(mod, x) for x in r]
        return [f[0] for f in forks], [f[1] for f in forks]
    scale = _droppath_scale_for(n, shortcut.shape[0], drop_prob, training, shortcut.device)
    outs = ResidualLayerNormMultiFn.apply(scale, mod.weight, mod.bias, mod.eps, out_dtype, n, shortcut, *branches)
    return list(outs[:n]), list(outs[n:])


def residual_layer_norm(mod: torch.nn.Module, shortcut: torch.Tensor, branch: torch.Tensor, drop_prob: float, training: bool, drop=None):
    """(x_new, mod(x_new)) with x_new = shortcut + DropPath(branch): the fused kernel when it applies (nn.LayerNorm over
    the last dim, branch already in the dtype the LayerNorm output takes), else residual_droppath + layer_norm_fork.  ``drop``: a
    pending activation dropout of the branch, as in ``residual_layer_norm_multi``."""
    C = shortcut.shape[-1]
    if drop is not None:
        return layer_norm_fork(mod, residual_droppath(shortcut, [branch], drop_prob, training, drop)[0])
    ok = (_ln_module_ok(mod, last_dim_only=True) and _ln_width_ok(shortcut, multiple=8, width=C)
          and branch.shape == shortcut.shape and shortcut.dim() == 3 and torch.is_grad_enabled() and (shortcut.requires_grad or branch.requires_grad))
    if ok:
        out_dtype = glue_dtype(shortcut)
        ok = branch.dtype == out_dtype
    if not ok:
        x = residual_droppath(shortcut, [branch], drop_prob, training)[0]
        return layer_norm_fork(mod, x)
    scale = _droppath_scale_for(1, shortcut.shape[0], drop_prob, training, shortcut.device)
    if scale is not None:
        scale = scale[0]
    return ResidualLayerNormFn.apply(shortcut, branch, scale, mod.weight, mod.bias, mod.eps, out_dtype)


def layer_norm_fork(mod: torch.nn.Module, x: torch.Tensor):
    """(x for the skip connection, LayerNorm(x) for the following linear): LayerNormFn's fork form.  Same dispatch rules as
    ``layer_norm`` (falls back to two separate uses of x when the fused kernel does not apply)."""
    y = layer_norm(mod, x, _fork=True)
    return y if isinstance(y, tuple) else (x, y)


def layer_norm_merge(mod: torch.nn.Module, x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """PatchMerging's ``norm(cat of the 2x2 neighbourhood)`` on a (B, H*W, C) token tensor -> (B, H*W/4, 4C): the gather is
    done by the LayerNorm kernels' addressing (forward reads, backward scatters), not by a strided copy.  Falls back to
    the explicit gather when the kernel does not apply."""
    B, _, C = x.shape
    if not _merge_ok(mod, x, H, W):
        g = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, (H // 2) * (W // 2), 4 * C)
        return layer_norm(mod, g)
    return LayerNormFn.apply(x, mod.weight, mod.bias, mod.eps, glue_dtype(x), (H, W))


class ResidualMergeNormStreamsFn(torch.autograd.Function):
    """PatchMerging's ``norm(2x2 neighbourhood concat)`` of n independent streams (B, H*W, C) at once -> ONE stacked
    (n*B, H*W/4, 4C) tensor (stream-major), so that the following reduction runs as a single GEMM over all streams.  One launch
    forward, one backward (+ reduce), dgamma / dbeta summed over the streams.  Two forms of the same kernels (csrc/layernorm.hip):
      * n tensors: the streams themselves are normalised (``mtlora_layernorm_multi_fwd/bwd``);
      * 2n tensors, res then branches: x_new_k = res_k + scale[k] * branch_k (MLP residual + DropPath of the task-enabled block) is
        formed first and kept for the backward only (``mtlora_residual_layernorm_streams_fwd/bwd``): d_branch_k = scale[k] * d_res_k.
    args: scale ((n, B) fp32 or None; None without branches), weight, bias, eps, out_dtype, H, W, n, *res(n) [, *branches(n)]"""

    @staticmethod
    def forward(ctx, scale, weight, bias, eps: float, out_dtype: torch.dtype, H: int, W: int, n: int, *tensors):
        res, brs = tensors[:n], tensors[n:]
        L.require_gpu(weight, bias, *tensors)
        B, Lt, Ct = res[0].shape
        C, M = 4 * Ct, B * Lt // 4
        r2 = [x.contiguous() for x in res]
        w, b = _ln_affine(weight, bias)
        y = torch.empty((n, M, C), dtype=out_dtype, device=r2[0].device)
        ys = [y[k] for k in range(n)]
        stats, means, rstds = _ln_stream_stats(n, M, r2[0].device)
        if brs:
            b2 = [x.contiguous() for x in brs]
            xs = [torch.empty_like(x) for x in r2]
            st = L.lib().mtlora_residual_layernorm_streams_fwd(n, L.ptr_array9(r2), L.ptr_array9(b2), L.ptr(scale), B, L.ptr(w), L.ptr(b),
                                                               L.ptr_array9(xs), L.ptr_array9(ys), L.ptr_array9(means),
                                                               L.ptr_array9(rstds), M, C, float(eps), L.dtype_code(r2[0]),
                                                               L.dtype_code(y), H, W, L.stream_ptr())
            L.check(st, "mtlora_residual_layernorm_streams_fwd")
            ctx.save_for_backward(w, stats, scale, *xs)
        else:
            st = L.lib().mtlora_layernorm_multi_fwd(n, L.ptr_array9(r2), L.ptr(w), L.ptr(b), L.ptr_array9(ys), L.ptr_array9(means),
                                                    L.ptr_array9(rstds), M, C, float(eps), L.dtype_code(r2[0]), L.dtype_code(y), H, W,
                                                    L.stream_ptr())
            L.check(st, "mtlora_layernorm_multi_fwd")
            ctx.save_for_backward(w, stats, None, *r2)
        ctx.cfg = (n, M, C, H, W, B, res[0].shape, brs[0].dtype if brs else None)
        return y.view(n * B, Lt // 4, C)

    @staticmethod
    def backward(ctx, g):
        w, stats, scale, *xs = ctx.saved_tensors
        n, M, C, H, W, B, shape, bdt = ctx.cfg
        # with branches the kernel writes their gradients (of their dtype) from g; without, it takes g's own dtype
        g3 = _canon_grad(g, (n, M, C), _kernel_dtype(g.dtype) if bdt is None else bdt)
        gs = [g3[k] for k in range(n)]
        scratch, sb, dg, db = _ln_bwd_buffers(M, C, xs[0], n)
        dres = [torch.empty_like(x) for x in xs]
        _, means, rstds = _ln_stream_stats(n, M, stats=stats)
        if bdt is None:
            st = L.lib().mtlora_layernorm_multi_bwd(n, L.ptr_array9(gs), L.ptr_array9(xs), L.ptr(w), L.ptr_array9(means),
                                                    L.ptr_array9(rstds), L.ptr_array9(dres), L.ptr(dg), L.ptr(db), M, C,
                                                    L.dtype_code(xs[0]), L.dtype_code(g3), L.ptr(scratch), sb, L.ptr_array9(None), H, W,
                                                    L.stream_ptr())
            L.check(st, "mtlora_layernorm_multi_bwd")
            return (None, dg, db, None, None, None, None, None, *[d.view(shape) for d in dres])
        dbr = [torch.empty(shape, dtype=bdt, device=xs[0].device) for _ in range(n)]
        st = L.lib().mtlora_residual_layernorm_streams_bwd(n, L.ptr_array9(gs), L.ptr_array9(xs), L.ptr(w), L.ptr_array9(means),
                                                           L.ptr_array9(rstds), L.ptr_array9(dres), L.ptr_array9(dbr), L.ptr(dg),
                                                           L.ptr(db), L.ptr(scale), B, M, C, L.dtype_code(xs[0]), L.dtype_code(g3),
                                                           L.ptr(scratch), sb, L.ptr_array9(None), H, W, L.stream_ptr())
        L.check(st, "mtlora_residual_layernorm_streams_bwd")
        return (None, dg, db, None, None, None, None, None, *[d.view(shape) for d in dres], *dbr)


def residual_merge_norm_streams(mod: torch.nn.Module, res, branches, H: int, W: int, drop_prob: float, training: bool):
    """stacked PatchMerging-norm of (res_k + DropPath_k(branches_k)) over the streams, or None when the fused kernels do not
    apply (the caller then forms the residuals and calls ``layer_norm_merge_multi`` / per-stream code)."""
    n = len(res)
    ok = (_streams_ok(res) and len(branches) == n
          and all(x.shape == res[0].shape and x.dtype == branches[0].dtype for x in branches)
          and _merge_ok(mod, res[0], H, W) and torch.is_grad_enabled())
    if ok:
        out_dtype = glue_dtype(res[0])
        ok = branches[0].dtype == out_dtype
    if not ok:
        return None
    scale = _droppath_scale_for(n, res[0].shape[0], drop_prob, training, res[0].device)
    return ResidualMergeNormStreamsFn.apply(scale, mod.weight, mod.bias, mod.eps, out_dtype, H, W, n, *res, *branches)


def layer_norm_merge_multi(mod: torch.nn.Module, xs, H: int, W: int):
    """stacked (n*B, H*W/4, 4C) = cat_k PatchMerging-norm(xs[k]) (stream-major), or None when the fused kernel does not apply."""
    if not (_streams_ok(xs) and _merge_ok(mod, xs[0], H, W)):
        return None
    return ResidualMergeNormStreamsFn.apply(None, mod.weight, mod.bias, mod.eps, glue_dtype(xs[0]), H, W, len(xs), *xs)


def layer_norm(mod: torch.nn.Module, x: torch.Tensor, feeds_linear: bool = True, _fork: bool = False):
    """``mod(x)`` for an ``nn.LayerNorm`` over the last dim, through the HIP kernel.  ``feeds_linear``: the output is
    only consumed by an MTLoRALinear, so it is written directly in the hot path's compute dtype (bf16 under autocast
    -- no fp32 intermediate + cast pass).  Otherwise (patch_embed.norm, whose output IS the residual stream) the
    output dtype is what the reference produces: fp32 under autocast (autocast runs layer_norm in fp32), else the
    input dtype.  Anything else (custom norm layers, no affine, exotic dtypes) goes to the module itself."""
    ok = _ln_module_ok(mod, last_dim_only=True) and _ln_width_ok(x, multiple=8, width=x.shape[-1])
    if not ok:
        return mod(x)
    if feeds_linear:
        out_dtype = glue_dtype(x)
    else:
        out_dtype = torch.float32 if torch.is_autocast_enabled() else x.dtype
    return LayerNormFn.apply(x, mod.weight, mod.bias, mod.eps, out_dtype, None, _fork and x.requires_grad)  # fork: (x_skip, y)


# ----------------------------------------------------------------------------------------------
# SHARED_MODE "addition" (reference lora.py:275-284): y + LayerNorm(sum of the task outputs), one kernel each way
# ----------------------------------------------------------------------------------------------
def sum_norm_add_torch(y: torch.Tensor, y_t, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    """The portable definition of ``mtlora_sum_ln_add_fwd``: ``y + LayerNorm(sum_k y_t[k])`` over the last dim, the sum taken
    in index order, everything carried in fp32 (in fp64 for fp64 inputs) and rounded to ``y.dtype`` once.  Plain torch, any device,
    differentiable."""
    acc = torch.promote_types(y.dtype, torch.float32)
    tot = y_t[0].to(acc)
    for t in y_t[1:]:
        tot = tot + t.to(acc)
    mean = tot.mean(-1, keepdim=True)
    d = tot - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    return (y.to(acc) + (d * rstd * weight.to(acc) + bias.to(acc))).to(y.dtype)


def sum_norm_add_ok(mod: torch.nn.Module, y: torch.Tensor, y_t) -> bool:
    """may ``SumNormAddFn`` take this call?  An affine ``nn.LayerNorm`` over the last dim, 1 .. MAX_TASKS task outputs, everything
    on the device, contiguous, of one kernel dtype and shape, the width a multiple of a 16-byte vector and at most 4096"""
    return (_ln_module_ok(mod, last_dim_only=True) and 1 <= len(y_t) <= L.MAX_TASKS and y.dim() >= 1 and y.is_contiguous()
            and _ln_width_ok(y, multiple=_ln_vec(y), width=y.shape[-1], cap=(4096, 4096)) and mod.weight.is_cuda
            and all(t.is_cuda and t.dtype == y.dtype and t.shape == y.shape and t.is_contiguous() for t in y_t))


class SumNormAddFn(torch.autograd.Function):
    """(out, y_t_0 .. y_t_n-1) = (y + LayerNorm(sum_k y_t_k), the task outputs passed through).  The task outputs leave the node
    again because they feed the LayerNorm AND whatever consumes them downstream (a fork, as ``LayerNormFn(fork=True)``): the
    backward kernel then forms  d y_t_k = g_k + LN-backward(g_out)  itself (``dy_t_addend``) instead of autograd's n full-size
    gradient adds.  The gradient of ``y`` is ``g_out``, passed through.  Saves y_t, mean and rstd; ``tot`` is formed again.
    args: y, weight, bias, eps, *y_t"""

    @staticmethod
    def forward(ctx, y, weight, bias, eps: float, *y_t):
        L.require_gpu(y, weight, bias, *y_t)
        n, N = len(y_t), y.shape[-1]
        M = y.numel() // N
        w, b = _ln_affine(weight, bias)
        out = torch.empty_like(y)
        mean, rstd = _ln_row_stats(M, y.device)
        st = L.lib().mtlora_sum_ln_add_fwd(n, L.ptr_array(y_t), L.ptr(y), L.ptr(w), L.ptr(b), L.ptr(out), L.ptr(mean),
                                                  L.ptr(rstd), M, N, float(eps), L.dtype_code(y), L.stream_ptr())
        L.check(st, "mtlora_sum_ln_add_fwd")
        ctx.save_for_backward(w, mean, rstd, *y_t)
        ctx.MN = (M, N)
        ctx.set_materialize_grads(False)
        return (out,) + tuple(t.view_as(t) for t in y_t)

    @staticmethod
    def backward(ctx, g_out, *g_t):
        w, mean, rstd, *y_t = ctx.saved_tensors
        M, N = ctx.MN
        n = len(y_t)
        if g_out is None:  # the sum was not used: the task outputs' own gradients pass through
            return (None, None, None, None) + tuple(g_t)
        dt, shape = y_t[0].dtype, y_t[0].shape
        dout = _canon_grad(g_out, shape, dt)
        adds = [_canon_grad(g, shape, dt) for g in g_t]
        want_affine = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        lib, code = L.lib(), L.dtype_code(dout)
        sb = lib.mtlora_sum_ln_add_bwd_scratch_bytes(n, M, N, code)
        scratch = _scratch(sb, dout.device, "sum + LayerNorm + add backward shape (n, M, N)", n, M, N)
        dg = torch.empty(N, dtype=torch.float32, device=dout.device) if want_affine else None
        db = torch.empty(N, dtype=torch.float32, device=dout.device) if want_affine else None
        dys = [torch.empty(shape, dtype=dt, device=dout.device) for _ in range(n)]
        st = lib.mtlora_sum_ln_add_bwd(n, L.ptr(dout), L.ptr_array(y_t), L.ptr(w), L.ptr(mean), L.ptr(rstd), L.ptr_array(adds),
                                              L.ptr_array(dys), L.ptr(dg), L.ptr(db), M, N, code, L.ptr(scratch), sb, L.stream_ptr())
        L.check(st, "mtlora_sum_ln_add_bwd")
        return (g_out, dg if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None) + tuple(dys)


# ----------------------------------------------------------------------------------------------
# training-mode BatchNorm (+ReLU) over a channels-last (rows, C) matrix (decoder heads)
# ----------------------------------------------------------------------------------------------
class BatchNormReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum: float, eps: float, relu: bool):
        L.require_gpu(x, weight, bias)
        R, C = x.shape
        x = x.contiguous()
        w, b = _f32_param(weight), _f32_param(bias)
        y = torch.empty_like(x)
        saves = torch.empty(4, C, dtype=torch.float32, device=x.device)  # mean, rstd, scale, shift
        lib = L.lib()
        sb = lib.mtlora_bn_scratch_bytes(R, C, L.dtype_code(x))
        scratch = _scratch(sb, x.device, "BatchNorm shape (rows, C, dtype)", R, C, x.dtype)
        st = lib.mtlora_bn_relu_fwd(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(running_mean), L.ptr(running_var), float(momentum),
                                    float(eps), int(relu), L.ptr(y), L.ptr(saves[0]), L.ptr(saves[1]), L.ptr(saves[2]),
                                    L.ptr(saves[3]), R, C, L.dtype_code(x), L.ptr(scratch), sb, L.stream_ptr())
        L.check(st, "mtlora_bn_relu_fwd")
        ctx.save_for_backward(x, saves)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, saves = ctx.saved_tensors
        R, C = x.shape
        dy = dy.to(x.dtype).contiguous()
        lib = L.lib()
        sb = lib.mtlora_bn_scratch_bytes(R, C, L.dtype_code(x))
        scratch = _scratch(sb, x.device, "BatchNorm shape (rows, C, dtype)", R, C, x.dtype)
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        st = lib.mtlora_bn_relu_bwd(L.ptr(dy), L.ptr(x), L.ptr(saves[0]), L.ptr(saves[1]), L.ptr(saves[2]), L.ptr(saves[3]),
                                    int(ctx.relu), L.ptr(dx), L.ptr(dg), L.ptr(db), R, C, L.dtype_code(x), L.ptr(scratch), sb,
                                    L.stream_ptr())
        L.check(st, "mtlora_bn_relu_bwd")
        return dx, dg, db, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# activation dropout (MODEL.DROP_RATE) generated inside the kernels: hidden / projection / Mlp output / position
# ----------------------------------------------------------------------------------------------
def act_dropout_stream(site: int, k: int) -> int:
    """generator stream of tensor ``k`` of a call at ``site`` (``L.ACT_DROP_*``): 0 the shared tensor, 1 + i task i"""
    return site + L.ACT_DROP_TENSOR_STRIDE * k


def act_dropout_keep(seed: int, site: int, k: int, rows: int, cols: int, p: float, device="cpu") -> torch.Tensor:
    """keep[m, c] (bool) of element (row m, channel c) of tensor ``k`` of a call at ``site``: the counter-based generator of
    csrc/common.h (``mtl_dropout_keep``) in int64 torch arithmetic, on any device -- the definition the kernels implement."""
    thr = min(int(p * 65536.0), 65535) if p > 0.0 else 0
    if thr == 0:
        return torch.ones(rows, cols, dtype=torch.bool, device=device)
    M32 = 0xFFFFFFFF

    def mix(x):  # x in [0, 2^32): int64 products wrap mod 2^64, the low 32 bits are exact
        x = x ^ (x >> 16)
        x = (x * 0x7FEB352D) & M32
        x = x ^ (x >> 15)
        x = (x * 0x846CA68B) & M32
        return x ^ (x >> 16)

    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    m = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(cols, dtype=torch.int64, device=device)[None, :]
    rh = mix((m * 0x9E3779B1 + seed_lo + act_dropout_stream(site, k) * 0x85EBCA77) & M32)
    h = mix(rh ^ (((c >> 1) + seed_hi * 0x27D4EB2F) & M32))
    bits = torch.where((c & 1) == 1, h >> 16, h & 0xFFFF)
    return bits >= thr


def _dropped(x: torch.Tensor, seed: int, site: int, k: int, p: float) -> torch.Tensor:
    C = x.shape[-1]
    keep = act_dropout_keep(seed, site, k, x.numel() // C, C, p, x.device).view(x.shape)
    on = p > 0.0 and int(p * 65536.0) > 0
    return torch.where(keep, x * (1.0 / (1.0 - p)) if on else x, torch.zeros((), dtype=x.dtype, device=x.device))


def act_dropout_torch(hs, act: int, p: float, seed: int, site: int):
    """portable definition of :class:`ActDropoutFn`: [keep_k * act(h_k) / (1 - p)] in plain torch (any device; ``seed`` is the
    effective seed, any device-side offset already added)"""
    return [_dropped(torch.nn.functional.gelu(h) if act == L.ACT_GELU else h, seed, site, k, p) for k, h in enumerate(hs)]


def residual_droppath_drop_torch(res, ys, scale, p: float, seed: int, site: int):
    """portable definition of ``residual_droppath(..., drop=(p, seed, site))``: [res_k + scale[k, sample] * keep_k * ys_k / (1 - p)];
    ``res`` one shared tensor or a list, ``scale`` (n, B) or None, ``seed`` the effective seed"""
    shared = not isinstance(res, (list, tuple))
    out = []
    for k, y in enumerate(ys):
        y = _dropped(y, seed, site, k, p)
        if scale is not None:
            y = y * scale[k].view(-1, *([1] * (y.ndim - 1))).to(y.dtype)
        out.append((res if shared else res[k]) + y)
    return out


def _effective_seed(seed: int) -> int:
    """host value of ``seed`` + the device seed-offset word (a synchronising read: portable fallbacks only)"""
    off = 0 if _seed_offset is None else int(_seed_offset.item())
    return (seed + off) & 0xFFFFFFFFFFFFFFFF


def _drop_arg(p: float, seed: int) -> "L.AttnDropout":
    dr = L.AttnDropout()
    dr.p, dr.seed, dr.seed_offset = p, seed, (0 if _seed_offset is None else _seed_offset.data_ptr())
    return dr


def act_dropout_ok(ts) -> bool:
    """may the activation-dropout kernels take these tensors?  On the GPU, contiguous, one kernel dtype and shape, width % 8 == 0"""
    t0 = ts[0]
    return (1 <= len(ts) <= L.MAX_TASKS + 1 and t0.is_cuda and t0.dtype in _GLUE_DTYPES and t0.dim() >= 2 and t0.shape[-1] % 8 == 0
            and t0.numel() // t0.shape[-1] < (1 << 32)
            and all(t.is_cuda and t.dtype == t0.dtype and t.shape == t0.shape and t.is_contiguous() for t in ts))


def pending_dropout(p: float, site: int):
    """a dropout that the consumer applies (``residual_droppath(..., drop=...)``): draws the call site's seed NOW, in forward order"""
    return (float(p), next_seed(), site)


class ActDropoutFn(torch.autograd.Function):
    """outs[k] = keep_k * act(hs[k]) / (1 - p) for the n tensors of a call site, one launch per direction; the backward reads the
    gradient (and h for GELU) and regenerates keep_k.  ``act``: ``L.ACT_IDENTITY`` / ``L.ACT_GELU`` (exact erf form); ``seed`` (plus the
    device word of :func:`set_seed_offset`) and the tensor's index select the mask (:func:`act_dropout_keep`).
    args: site, act, p, seed, *hs"""

    @staticmethod
    def forward(ctx, site: int, act: int, p: float, seed: int, *hs):
        L.require_gpu(*hs)
        n, C = len(hs), hs[0].shape[-1]
        M = hs[0].numel() // C
        hc = [h.contiguous() for h in hs]
        outs = [torch.empty_like(h) for h in hc]
        dr = _drop_arg(float(p), int(seed))
        st = L.lib().mtlora_act_dropout_fwd(n, L.ptr_array9(hc), L.ptr_array9(outs), ctypes.byref(dr), site, act, M, C,
                                            L.dtype_code(hc[0]), L.stream_ptr())
        L.check(st, "mtlora_act_dropout_fwd")
        ctx.cfg = (site, act, n, M, C, hc[0].dtype, dr, _seed_offset)
        if act != L.ACT_IDENTITY:
            ctx.save_for_backward(*hc)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        site, act, n, M, C, dt, dr, _ = ctx.cfg
        hc = ctx.saved_tensors
        gs = [g.to(dt).contiguous() for g in grads]
        dhs = [torch.empty_like(g) for g in gs]
        st = L.lib().mtlora_act_dropout_bwd(n, L.ptr_array9(gs), L.ptr_array9(hc), L.ptr_array9(dhs), ctypes.byref(dr),
                                            site, act, M, C, L._DT[dt], L.stream_ptr())
        L.check(st, "mtlora_act_dropout_bwd")
        return (None, None, None, None, *dhs)


def apply_pending_dropout(ts, drop):
    """a pending dropout (``pending_dropout``) applied as a launch of its own: the same mask the residual kernel would have used"""
    return list(ActDropoutFn.apply(drop[2], L.ACT_IDENTITY, drop[0], drop[1], *ts))


def act_dropout(ts, act: int, p: float, site: int):
    """[drop(act(t))] for the tensors of one call site through :class:`ActDropoutFn` (one seed for the call), or None when the
    kernels do not take them (the caller's nn.Dropout path then runs, and no seed has been drawn)"""
    if not act_dropout_ok(ts):
        return None
    return list(ActDropoutFn.apply(site, act, float(p), next_seed(), *ts))


# ----------------------------------------------------------------------------------------------
# residual + DropPath over the 1+T tensors of a block half
# ----------------------------------------------------------------------------------------------
class ResidualDropPathFn(torch.autograd.Function):
    """outs[k] = res[k] + scale[k, sample] * ys[k].
    args: scale ((n, B) fp32 or None), shared (bool: every k adds the SAME residual tensor res[0]), n,
          *res (1 tensor if shared else n), *ys (n) [, p, seed, site].
    Optional ``p, seed, site``: dropout on the branches (``proj_drop`` / the Mlp's output drop) generated inside the kernels --
    outs[k] = res[k] + scale[k, sample] * keep[k] / (1 - p) * ys[k], keep[k] as :func:`act_dropout_keep` defines it for tensor k."""

    @staticmethod
    def forward(ctx, scale, shared: bool, n: int, *tensors):
        nres = 1 if shared else n
        res, ys = list(tensors[:nres]), list(tensors[nres:nres + n])
        L.require_gpu(*res, *ys)
        B = res[0].shape[0]
        C = res[0].shape[-1]
        M = res[0].numel() // C
        res_c = [r.contiguous() for r in res]
        ys_c = [y.contiguous() for y in ys]
        outs = [torch.empty_like(res_c[0]) for _ in range(n)]
        rlist = res_c * n if shared else res_c
        drop = tensors[nres + n:]
        if drop and float(drop[0]) > 0.0:  # dropout on the branches, generated in the kernel (row = row of the (M, C) matrix)
            dr, site = _drop_arg(float(drop[0]), int(drop[1])), int(drop[2])
            st = L.lib().mtlora_residual_droppath_drop_fwd(n, L.ptr_array9(rlist), L.ptr_array9(ys_c), L.ptr_array9(outs), L.ptr(scale),
                                                           ctypes.byref(dr), site, M, C, B, L.dtype_code(res_c[0]),
                                                           L.dtype_code(ys_c[0]), L.stream_ptr())
            L.check(st, "mtlora_residual_droppath_drop_fwd")
            ctx.drop = (dr, site, _seed_offset)
        else:
            st = L.lib().mtlora_residual_droppath_fwd(n, L.ptr_array9(rlist), L.ptr_array9(ys_c), L.ptr_array9(outs), L.ptr(scale),
                                                      M, C, B, L.dtype_code(res_c[0]), L.dtype_code(ys_c[0]), L.stream_ptr())
            L.check(st, "mtlora_residual_droppath_fwd")
            ctx.drop = None
        ctx.n_drop = len(drop)
        ctx.cfg = (shared, n, M, C, B, res_c[0].dtype, ys_c[0].dtype, res_c[0].shape)
        ctx.save_for_backward(scale)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        shared, n, M, C, B, rdt, ydt, shape = ctx.cfg
        (scale,) = ctx.saved_tensors
        if all(g is None for g in grads):
            return (None,) * (3 + (1 if shared else n) + n + ctx.n_drop)
        dev = next(g for g in grads if g is not None).device
        gs = [None if g is None else g.to(rdt).contiguous() for g in grads]
        dys = [None if g is None else torch.empty(shape, dtype=ydt, device=dev) for g in gs]
        dres = torch.empty(shape, dtype=rdt, device=dev) if shared else None
        rcode = L.dtype_code(gs[[g is not None for g in gs].index(True)])
        if ctx.drop is not None:
            st = L.lib().mtlora_residual_droppath_drop_bwd(n, L.ptr_array9(gs), L.ptr_array9(dys), L.ptr(dres), L.ptr(scale),
                                                           ctypes.byref(ctx.drop[0]), ctx.drop[1], M, C, B, rcode, L._DT.get(ydt, L.F32),
                                                           L.stream_ptr())
            L.check(st, "mtlora_residual_droppath_drop_bwd")
        else:
            st = L.lib().mtlora_residual_droppath_bwd(n, L.ptr_array9(gs), L.ptr_array9(dys), L.ptr(dres), L.ptr(scale), M, C, B,
                                                      rcode, L._DT.get(ydt, L.F32), L.stream_ptr())
            L.check(st, "mtlora_residual_droppath_bwd")
        dres_out = [dres] if shared else gs          # separate residuals: identity (the incoming gradient itself)
        return (None, None, None, *dres_out, *dys) + (None,) * ctx.n_drop


def residual_droppath(res, ys, drop_prob: float, training: bool, drop=None):
    """[res_k + DropPath(ys_k)] for k in range(len(ys)) with an independent per-sample mask per k (timm DropPath,
    scale_by_keep).  ``res``: one tensor shared by all k, or a list of len(ys) tensors.  ``drop``: a pending activation dropout
    ``(p, seed, site)`` of the branches (``pending_dropout``), applied to ys_k before DropPath inside the same kernel."""
    shared = not isinstance(res, (list, tuple))
    rl = [res] if shared else list(res)
    n = len(ys)
    ok = (rl[0].is_cuda and rl[0].shape[-1] % 8 == 0 and all(t.dtype in _GLUE_DTYPES for t in rl + list(ys))
          and len({t.dtype for t in rl}) == 1 and len({t.dtype for t in ys}) == 1 and n <= L.MAX_TASKS + 1
          and all(t.shape == rl[0].shape for t in list(ys) + rl))
    scale = _droppath_scale_for(n, rl[0].shape[0], drop_prob, training, rl[0].device)
    if not ok:
        if drop is not None:
            return residual_droppath_drop_torch(res, ys, scale, drop[0], _effective_seed(drop[1]), drop[2])
        out = []
        for k in range(n):
            y = ys[k] if scale is None else ys[k] * scale[k].view(-1, *([1] * (ys[k].ndim - 1))).to(ys[k].dtype)
            out.append((rl[0] if shared else rl[k]) + y)
        return out
    if drop is not None:
        return list(ResidualDropPathFn.apply(scale, shared, n, *rl, *ys, *drop))
    return list(ResidualDropPathFn.apply(scale, shared, n, *rl, *ys))


def column_sum(g2: torch.Tensor) -> torch.Tensor:
    """fp32 ``g2.sum(0)`` of a contiguous (M, N) fp32 / bf16 matrix through ``mtlora_colsum`` (deterministic, two launches, no
    device memset: ATen's multi-block reduce zeroes a semaphore buffer first, which a HIP-graph capture of the step cannot
    replay on this stack); shapes the kernel does not take fall back to ATen."""
    M, N = g2.shape
    ve = 4 if g2.dtype == torch.float32 else 8
    if g2.dtype not in (torch.float32, torch.bfloat16) or N % ve or not g2.is_contiguous() or M == 0:
        return g2.sum(0, dtype=torch.float32)
    lib = L.lib()
    sb = lib.mtlora_colsum_scratch_bytes(M, N)
    scratch = _scratch(sb, g2.device, "column-sum shape (M, N)", M, N)
    out = torch.empty(N, dtype=torch.float32, device=g2.device)
    L.check(lib.mtlora_colsum(L.ptr(g2), M, N, L.dtype_code(g2), L.ptr(out), L.ptr(scratch), sb, L.stream_ptr()), "mtlora_colsum")
    return out


def label_stat(lab: torch.Tensor, kind: int, ignore_index: float) -> torch.Tensor:
    """label-only statistic of the fused losses as a 1-element fp32 tensor (kind 0: #{lab != ignore_index}; kind 1:
    mean(1 - (lab >= 0.5))) through ``mtlora_label_stat`` (see ``column_sum`` for why not ATen)."""
    n = lab.numel()
    lib = L.lib()
    sb = lib.mtlora_label_stat_scratch_bytes(n)
    scratch = _scratch(sb, lab.device, "label count", n)
    out = torch.empty(1, dtype=torch.float32, device=lab.device)
    L.check(lib.mtlora_label_stat(L.ptr(lab), n, kind, float(ignore_index), L.ptr(out), L.ptr(scratch), sb, L.stream_ptr()),
            "mtlora_label_stat")
    return out


def _valid_flags(valid, B: int, device) -> torch.Tensor:
    """``valid`` checked as the contiguous uint8 (B,) device tensor the kernels read; it passes through as it is, never as a
    copy: a static buffer stays the buffer a captured launch reads"""
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or tuple(valid.shape) != (B,):
        raise RuntimeError(f"mtlora_amd: valid must be a uint8 tensor of shape ({B},), got "
                           f"{getattr(valid, 'dtype', type(valid))} {tuple(getattr(valid, 'shape', ()))}")
    if valid.device != device:
        raise RuntimeError(f"mtlora_amd: valid lives on {valid.device}, the prediction on {device}")
    if not valid.is_contiguous():  # (a copy would be what a captured launch reads from then on, not the caller's buffer)
        raise RuntimeError("mtlora_amd: valid must be contiguous (the kernels read the tensor itself, also at replay time)")
    return valid


def label_stat_valid(lab: torch.Tensor, valid: Optional[torch.Tensor], kind: int, ignore_index: float) -> torch.Tensor:
    """``label_stat`` over the labelled samples of a batch, as a 2-element fp32 tensor ``[statistic, |V|]`` through
    ``mtlora_label_stat_valid``: ``lab`` (B, ...) contiguous fp32, ``valid`` uint8 (B,) on the same device (non-zero: the sample
    has a label; ``None``: all have).  ``kind`` 0 / 1 as ``label_stat``, 2: only ``|V|`` (the statistic is 0, the labels are not
    read).  The labels of an unlabelled sample are never read; nothing comes back to the host."""
    B = lab.shape[0]
    nps = lab.numel() // max(B, 1)
    lib = L.lib()
    sb = lib.mtlora_label_stat_valid_scratch_bytes(B, nps)
    scratch = _scratch(sb, lab.device, "label count per sample", B, nps)
    out = torch.empty(2, dtype=torch.float32, device=lab.device)
    v = None if valid is None else _valid_flags(valid, B, lab.device)
    L.check(lib.mtlora_label_stat_valid(L.ptr(lab), None if v is None else L.ptr(v), B, nps, kind, float(ignore_index), L.ptr(out),
                                        L.ptr(scratch), sb, L.stream_ptr()), "mtlora_label_stat_valid")
    return out


# ----------------------------------------------------------------------------------------------
# loss end of the train step: bilinear upsample (integer scale, align_corners=False) + per-task loss, fused
# ----------------------------------------------------------------------------------------------
LOSS_KINDS = {"softmax": 0, "normals": 1, "balanced_bce": 2, "l1_masked": 3}


def loss_of_kind(kind: str, up: torch.Tensor, label: torch.Tensor, ignore_index: float = 255.0, pos_weight: Optional[float] = None):
    """the four criteria behind ``LOSS_KINDS`` on a full-resolution prediction ``up`` (B, C, H, W), in the dtype of ``up`` (fp64
    for an oracle), sync-free restatements of mtl_loss_schemes.py: same value, no .item() / masked_select host round trip.
    The one copy of the formulas: ``mtl_harness.task_loss`` applies them to the fp32 prediction."""
    if kind == "softmax":                           # SoftMaxwithLoss (:22-39)
        return F.nll_loss(F.log_softmax(up, 1), label[:, 0].long(), ignore_index=int(ignore_index))
    if kind == "normals":                           # NormalsLoss(normalize=True, L1, size_average) (:162-220)
        mask = (label != ignore_index).to(up.dtype)
        on = up / (torch.norm(up, p=2, dim=1, keepdim=True) + 1e-12)
        return ((on - label).abs() * mask).sum() / mask.sum().clamp_min(1e-6)
    if kind == "balanced_bce":                      # BalancedCrossEntropyLoss(size_average[, pos_weight]) (:42-89, :243-245)
        labels = (label >= 0.5).to(up.dtype)
        w = (1.0 - labels).sum() / labels.numel() if pos_weight is None else float(pos_weight)
        gz = (up >= 0).to(up.dtype)
        lv = up * (labels - gz) - torch.log(1 + torch.exp(up - 2 * up * gz))
        return (w * (-(labels * lv)).sum() + (1 - w) * (-((1.0 - labels) * lv)).sum()) / labels.numel()
    if kind == "l1_masked":                         # DepthLoss l1 (:132-148)
        mask = (label != ignore_index).to(up.dtype)
        return ((up - label).abs() * mask).sum() / mask.sum().clamp_min(1.0)
    raise RuntimeError(f"mtlora_amd: unknown fused loss kind {kind!r}")


def upsample_loss_valid_torch(kind: str, low, label, scale: int, valid=None, ignore_index: float = 255.0,
                              pos_weight: Optional[float] = None):
    """The semantics of ``UpsampleLossFn.apply(..., valid=valid)`` in plain torch, on any device and in the dtype of ``low`` (fp64
    for an oracle): the samples with ``valid[b] != 0`` are index-selected, their low-resolution prediction is upsampled
    (bilinear, align_corners=False) and the criterion of ``kind`` is applied to that sub-batch -- what the reference's
    ``criterion(pred[V], gt[V])`` computes.  No labelled sample: ``+0.0`` with a zero gradient (the reference would divide by
    zero).  Unlabelled samples' ``low`` and ``label`` are never touched, so they may hold anything.  ``valid=None``: all labelled.
    The documented definition and the tests' oracle; it reads ``valid`` on the host."""
    B = low.shape[0]
    if valid is None:
        idx = torch.arange(B, device=low.device)
    else:
        idx = torch.nonzero(torch.as_tensor(valid).reshape(-1) != 0).reshape(-1).to(low.device)
    if idx.numel() == 0:
        return low.reshape(-1)[:0].sum()  # +0.0, differentiable: d / d low = 0
    lo = low.index_select(0, idx)
    up = F.interpolate(lo.permute(0, 3, 1, 2), scale_factor=int(scale), mode="bilinear", align_corners=False)
    return loss_of_kind(kind, up, label.index_select(0, idx.to(label.device)), ignore_index, pos_weight)


class UpsampleLossFn(torch.autograd.Function):
    """loss_kind( F.interpolate(low.permute(0,3,1,2), scale_factor=scale, mode="bilinear"), label ) as ONE kernel that also
    produces d loss / d low (csrc/loss.hip); the upsampled prediction never exists.  ``low`` is (B, h, w, C)
    channels-last (fp32 / bf16), ``label`` (B, 1 | C, scale*h, scale*w).  ``pos_weight`` (``balanced_bce`` only): the constant
    weight of BalancedCrossEntropyLoss(pos_weight=...) instead of the label statistic (edge: 0.95).

    ``valid`` (uint8 (B,) on the device, non-zero: the sample carries a label for this task): the loss of the labelled
    sub-batch, ``upsample_loss_valid_torch``; the same launch (``mtlora_upsample_loss_valid``) fed by ``label_stat_valid``.  The
    kernels read the flags on the device -- a captured call follows the tensor's content at replay time -- and never read the
    prediction or the label of an unlabelled sample; its rows of d loss / d low are +0.0, and with no labelled sample the loss
    is +0.0.  ``None``: today's launch, bit for bit."""

    @staticmethod
    def forward(ctx, kind: str, low, label, scale: int, ignore_index: float = 255.0, pos_weight: Optional[float] = None,
                valid=None):
        L.require_gpu(low, label)
        B, h, w, C = low.shape
        H, W = h * scale, w * scale
        lab = label.detach().float().contiguous()
        exp_c = C if kind == "normals" else 1
        if tuple(lab.shape) != (B, exp_c, H, W):
            raise RuntimeError(f"mtlora_amd: label shape {tuple(lab.shape)} does not match prediction {(B, exp_c, H, W)}")
        lo = low.detach().contiguous()
        if lo.dtype not in (torch.float32, torch.bfloat16):
            lo = lo.float()
        if kind not in LOSS_KINDS:
            raise RuntimeError(f"mtlora_amd: unknown fused loss kind {kind!r}")
        vflags = None if valid is None else _valid_flags(valid, B, lo.device)
        # label-only statistics (independent of the prediction)
        if vflags is not None:  # [statistic over the labelled samples, their number]
            if kind == "balanced_bce" and pos_weight is not None:
                stat = torch.cat([torch.full((1,), float(pos_weight), dtype=torch.float32, device=lab.device),
                                  label_stat_valid(lab, vflags, 2, ignore_index)[1:]])
            else:
                stat = label_stat_valid(lab, vflags, 1 if kind == "balanced_bce" else 0, ignore_index)
        elif kind == "softmax":
            stat = label_stat(lab, 0, ignore_index)
        elif kind == "normals":
            stat = label_stat(lab, 0, ignore_index)
        elif kind == "balanced_bce":
            stat = (label_stat(lab, 1, ignore_index) if pos_weight is None
                    else torch.full((1,), float(pos_weight), dtype=torch.float32, device=lab.device))
        else:
            stat = label_stat(lab, 0, ignore_index)
        if pos_weight is not None and kind != "balanced_bce":
            raise RuntimeError(f"mtlora_amd: pos_weight applies to 'balanced_bce', not {kind!r}")
        lib = L.lib()
        n = lib.mtlora_upsample_loss_partials(B, h, w, int(scale))
        if n < 0:
            raise RuntimeError(f"mtlora_amd: fused upsample + loss supports scales 1..32, got {scale}")
        part = torch.empty(max(n, 1), dtype=torch.float32, device=lo.device)
        dlow = torch.empty_like(lo)
        if vflags is None:
            st = lib.mtlora_upsample_loss(LOSS_KINDS[kind], L.ptr(lo), L.ptr(lab), L.ptr(stat), L.ptr(dlow), L.ptr(part), B, h, w,
                                          C, int(scale), L.dtype_code(lo), float(ignore_index), L.stream_ptr())
            L.check(st, "mtlora_upsample_loss")
        else:
            st = lib.mtlora_upsample_loss_valid(LOSS_KINDS[kind], L.ptr(lo), L.ptr(lab), L.ptr(vflags), L.ptr(stat), L.ptr(dlow),
                                                L.ptr(part), B, h, w, C, int(scale), L.dtype_code(lo), float(ignore_index),
                                                L.stream_ptr())
            L.check(st, "mtlora_upsample_loss_valid")
        ctx.save_for_backward(dlow)
        ctx.in_dtype = low.dtype
        return part[:n].sum() if n > 0 else part.sum() * 0

    @staticmethod
    def backward(ctx, g):
        (dlow,) = ctx.saved_tensors
        return None, (dlow * g.to(dlow.dtype)).to(ctx.in_dtype), None, None, None, None, None


# validation end: bilinear upsample + get_output + meter update + loss, fused and forward-only (csrc/metrics.hip)
METRIC_KINDS = {"softmax": 0, "normals": 1, "saliency": 2, "l1_masked": 3, "edge": 4}
METRIC_FLOATS = {"softmax": 1, "normals": 3, "saliency": 1, "l1_masked": 3, "edge": 2}  # float quantities per kind, loss first
SAL_THRESHOLDS = 15, 19
_sal_thr: dict = {}


def saliency_thresholds(device=None):
    """the 15 + 19 thresholds of the reference's two saliency meters as the fp32 values its comparisons see:
    ``np.linspace(0.2, 0.9, 15)`` compared as Python floats against fp32 tensors (eval_sal_no_beta.py:27), and
    ``torch.arange(0.05, 1, 0.05)`` (eval_sal_beta.py:23).  Built on the CPU once; cached per device."""
    key = str(device)
    if key not in _sal_thr:
        import numpy as np
        t = torch.cat([torch.tensor(np.linspace(0.2, 0.9, 15), dtype=torch.float64).float(), torch.arange(0.05, 1, 0.05)])
        _sal_thr[key] = t if device is None else t.to(device)
    return _sal_thr[key]


def upsample_metrics_sizes(kind: str, B: int, h: int, w: int, C: int, scale: int):
    """(number of int64 counts, number of fp32 partials) of ``upsample_metrics``; pure host call, raises on a geometry the
    kernel does not take."""
    ni, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(L.lib().mtlora_upsample_metrics_sizes(METRIC_KINDS[kind], B, h, w, C, int(scale), ctypes.byref(ni), ctypes.byref(nf)),
            "mtlora_upsample_metrics_sizes")
    return ni.value, nf.value


@torch.no_grad()
def upsample_metrics(kind: str, low, label, scale: int, counts=None, ignore_index: float = 255.0, pos_weight: float = 0.95,
                     valid=None):
    """meter counters and loss of ``F.interpolate(low.permute(0,3,1,2), scale_factor=scale, mode="bilinear")`` against ``label``
    in ONE launch (csrc/metrics.hip; layouts in include/mtlora_hip.h).  ``low`` (B, h, w, C) channels-last fp32 / bf16.
    Returns ``(counts, sums)``: ``counts`` int64 -- the given tensor, ADDED to in place, or a fresh zeroed one -- and ``sums``
    the kind's float quantities as fp64 (loss first), summed over the tiles' partials in a fixed order.  No host sync.

    ``valid`` (uint8 (B,) on the device, non-zero: the sample carries a label for this task): counters, sums and loss of the
    labelled sub-batch ``(low[V], label[V])`` through ``mtlora_upsample_metrics_valid`` fed by ``label_stat_valid``; layouts
    and sizes stay those of the whole batch (an unlabelled image's saliency rows receive nothing).  The kernels read the flags
    on the device -- a captured call follows the tensor's content at replay time -- and never read the prediction or the label
    of an unlabelled sample; with no labelled sample ``counts`` is unchanged and every sum is +0.0.  ``None``: today's launch,
    bit for bit."""
    L.require_gpu(low, label)
    B, h, w, C = low.shape
    H, W = h * scale, w * scale
    lab = label.detach().float().contiguous()
    exp_c = C if kind == "normals" else 1
    if tuple(lab.shape) != (B, exp_c, H, W):
        raise RuntimeError(f"mtlora_amd: label shape {tuple(lab.shape)} does not match prediction {(B, exp_c, H, W)}")
    lo = low.detach().contiguous()
    if lo.dtype not in (torch.float32, torch.bfloat16):
        lo = lo.float()
    vflags = None if valid is None else _valid_flags(valid, B, lo.device)
    if kind not in METRIC_KINDS:
        raise RuntimeError(f"mtlora_amd: unknown fused metrics kind {kind!r}")
    if vflags is not None:  # the unmasked launch's words over the labelled samples, then their number |V|
        if kind == "saliency":
            sv = label_stat_valid(lab, vflags, 1, ignore_index)
            stat = torch.cat([sv[:1], saliency_thresholds(lab.device), sv[1:]])
        elif kind == "edge":
            stat = torch.cat([torch.full((1,), float(pos_weight), dtype=torch.float32, device=lab.device),
                              label_stat_valid(lab, vflags, 2, ignore_index)[1:]])
        else:
            stat = label_stat_valid(lab, vflags, 0, ignore_index)
    elif kind in ("softmax", "normals", "l1_masked"):
        stat = label_stat(lab, 0, ignore_index)
    elif kind == "saliency":
        stat = torch.cat([label_stat(lab, 1, ignore_index), saliency_thresholds(lab.device)])
    elif kind == "edge":
        stat = torch.full((1,), float(pos_weight), dtype=torch.float32, device=lab.device)
    else:
        raise RuntimeError(f"mtlora_amd: unknown fused metrics kind {kind!r}")
    ni, nfp = upsample_metrics_sizes(kind, B, h, w, C, scale)
    if counts is None:
        counts = torch.zeros(max(ni, 1), dtype=torch.int64, device=lo.device)
    elif counts.dtype != torch.int64 or counts.numel() < ni or not counts.is_contiguous() or counts.device != lo.device:
        raise RuntimeError(f"mtlora_amd: counts must be a contiguous int64 tensor of at least {ni} elements on {lo.device}")
    nq = METRIC_FLOATS[kind]
    part = torch.empty(max(nfp, nq), dtype=torch.float32, device=lo.device)
    if vflags is None:
        st = L.lib().mtlora_upsample_metrics(METRIC_KINDS[kind], L.ptr(lo), L.ptr(lab), L.ptr(stat), L.ptr(counts), L.ptr(part), B,
                                             h, w, C, int(scale), L.dtype_code(lo), float(ignore_index), L.stream_ptr())
        L.check(st, "mtlora_upsample_metrics")
    else:
        st = L.lib().mtlora_upsample_metrics_valid(METRIC_KINDS[kind], L.ptr(lo), L.ptr(lab), L.ptr(vflags), L.ptr(stat),
                                                   L.ptr(counts), L.ptr(part), B, h, w, C, int(scale), L.dtype_code(lo),
                                                   float(ignore_index), L.stream_ptr())
        L.check(st, "mtlora_upsample_metrics_valid")
    if nfp == 0:
        return counts, torch.zeros(nq, dtype=torch.float64, device=lo.device)
    return counts, part[:nfp].view(nq, nfp // nq).sum(1, dtype=torch.float64)


PREDICT_KINDS = {"argmax": 0, "normals": 1, "sigmoid": 2, "identity": 3}
_PREDICT_OUT = {"argmax": (torch.uint8,), "normals": (torch.float32, torch.uint8), "sigmoid": (torch.float32, torch.uint8),
                "identity": (torch.float32,)}  # the kind's output dtypes, default first


@torch.no_grad()
def upsample_predict(kind: str, low, scale: int, out_dtype=None, out=None):
    """``get_output(F.interpolate(low.permute(0,3,1,2), scale_factor=scale, mode="bilinear"), task)`` in ONE launch
    (csrc/predict.hip; include/mtlora_hip.h): ``low`` (B, h, w, C) channels-last fp32 / bf16 / fp16, the result at H = scale h,
    W = scale w.  ``argmax``: uint8 (B, H, W) class ids; ``normals``: (B, H, W, C) in [0, 255]; ``sigmoid``: (B, H, W) in
    [0, 255]; ``identity``: fp32 (B, H, W, 1).  ``out_dtype`` of normals / sigmoid: fp32 (default, get_output's values) or uint8
    (truncated, as ``.to(torch.uint8)``).  ``out``: a contiguous tensor of that shape and dtype to write into.  No host sync."""
    if kind not in PREDICT_KINDS:
        raise RuntimeError(f"mtlora_amd: unknown fused prediction kind {kind!r}")
    L.require_gpu(low, out)
    B, h, w, C = low.shape
    H, W = h * int(scale), w * int(scale)
    if out_dtype is None:
        out_dtype = _PREDICT_OUT[kind][0] if out is None else out.dtype
    if out_dtype not in _PREDICT_OUT[kind]:
        raise RuntimeError(f"mtlora_amd: fused prediction kind {kind!r} writes {_PREDICT_OUT[kind]}, not {out_dtype}")
    shape = {"argmax": (B, H, W), "normals": (B, H, W, C), "sigmoid": (B, H, W), "identity": (B, H, W, 1)}[kind]
    lo = low.detach().contiguous()
    if lo.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        lo = lo.float()
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=lo.device)
    elif tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != lo.device:
        raise RuntimeError(f"mtlora_amd: out must be a contiguous {out_dtype} tensor of shape {shape} on {lo.device}")
    st = L.lib().mtlora_upsample_predict(PREDICT_KINDS[kind], L.ptr(lo), L.ptr(out), B, h, w, C, int(scale), L.dtype_code(lo),
                                         L.U8 if out_dtype == torch.uint8 else L.F32, L.stream_ptr())
    L.check(st, "mtlora_upsample_predict")
    return out


# ----------------------------------------------------------------------------------------------
# batch ingest: wire-format tensors on the device -> the fp32 (B, C, H, W) tensors of the steps (csrc/ingest.hip)
# ----------------------------------------------------------------------------------------------
INGEST_KINDS = {"image": L.INGEST_IMAGE, "class": L.INGEST_CLASS, "class_allzero_ignore": L.INGEST_CLASS_ALLZERO_IGNORE,
                "normals": L.INGEST_NORMALS, "depth": L.INGEST_DEPTH}
_INGEST_SRC = {torch.uint8: L.U8, torch.float32: L.F32, torch.float16: L.F16}


def ingest_batch(jobs, flip=None, lut=None):
    """one ``mtlora_ingest_batch`` call (include/mtlora_hip.h) on the current stream: ``jobs`` is a sequence of
    ``(kind, src)`` with ``kind`` in ``INGEST_KINDS`` and ``src`` a contiguous device tensor in wire format -- image uint8
    (B, H, W, 3), class maps uint8 (B, H, W), normals fp32 / fp16 (B, H, W, 3), depth fp32 (B, H, W) -- all of one B, H, W;
    ``flip`` uint8 (B,) or None; ``lut`` the (3, 256) fp32 table of the image job (data.image_table).  Allocates the outputs
    (fp32 (B, C, H, W), returned in job order) and the flag scratch.  The library validates kinds, dtypes and channel counts;
    no host sync."""
    jobs = list(jobs)
    srcs = [s for _, s in jobs]
    L.require_gpu(*srcs, flip, lut)
    if not jobs:
        raise RuntimeError("mtlora_amd: ingest_batch needs at least one job")
    B, H, W = srcs[0].shape[:3]
    arr = (L.IngestJob * max(len(jobs), 1))()
    outs = []
    for i, (kind, src) in enumerate(jobs):
        if kind not in INGEST_KINDS:
            raise RuntimeError(f"mtlora_amd: unknown ingest kind {kind!r}")
        C = src.shape[3] if src.dim() == 4 else 1
        if src.dim() not in (3, 4) or tuple(src.shape[:3]) != (B, H, W) or not src.is_contiguous():
            raise RuntimeError(f"mtlora_amd: ingest job {i} ({kind}) must be a contiguous (B, H, W[, C]) tensor with "
                               f"B, H, W = {(B, H, W)}, got {tuple(src.shape)}")
        if src.dtype not in _INGEST_SRC:
            raise RuntimeError(f"mtlora_amd: unsupported dtype {src.dtype} for an ingest source (uint8, fp32 and fp16 are supported)")
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
        outs.append(out)
        arr[i].src, arr[i].dst, arr[i].kind, arr[i].src_dtype, arr[i].C = src.data_ptr(), out.data_ptr(), INGEST_KINDS[kind], \
            _INGEST_SRC[src.dtype], C
    if flip is not None and (flip.dtype != torch.uint8 or tuple(flip.shape) != (B,) or not flip.is_contiguous()):
        raise RuntimeError(f"mtlora_amd: flip must be a contiguous uint8 tensor of shape ({B},)")
    if lut is not None and (lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or not lut.is_contiguous()):
        raise RuntimeError("mtlora_amd: lut must be a contiguous fp32 tensor of shape (3, 256)")
    scratch, nbytes = None, 0
    if any(kind == "class_allzero_ignore" for kind, _ in jobs):
        nbytes = int(L.lib().mtlora_ingest_scratch_bytes(len(jobs), B))
        if nbytes > 0:
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=srcs[0].device)
    st = L.lib().mtlora_ingest_batch(arr, len(jobs), B, H, W, L.ptr(flip), L.ptr(lut), L.ptr(scratch), nbytes, L.stream_ptr())
    L.check(st, "mtlora_ingest_batch")
    return outs


# ----------------------------------------------------------------------------------------------
# geometric augmentation: raw canvas-format tensors on the device -> wire-format tensors at the output size (csrc/augment.hip)
# ----------------------------------------------------------------------------------------------
AUGMENT_KINDS = {"image_cubic_u8": L.AUGMENT_IMAGE_CUBIC_U8, "class_nearest_u8": L.AUGMENT_CLASS_NEAREST_U8,
                 "normals_cubic_f32": L.AUGMENT_NORMALS_CUBIC_F32, "depth_nearest_f32": L.AUGMENT_DEPTH_NEAREST_F32}
_AUGMENT_FORM = {"image_cubic_u8": (torch.uint8, 3), "class_nearest_u8": (torch.uint8, 1), "normals_cubic_f32": (torch.float32, 3),
                 "depth_nearest_f32": (torch.float32, 1)}


def augment_batch(jobs, size, coef, side, out_size, cubic_q15=None, cubic_f32=None, renormalize=True):
    """one ``mtlora_augment_batch`` call (include/mtlora_hip.h) on the current stream: ``jobs`` is a sequence of ``(kind, src)``
    with ``kind`` in ``AUGMENT_KINDS`` and ``src`` a contiguous device tensor on the canvas -- image uint8 (B, Hc, Wc, 3), class
    maps uint8 (B, Hc, Wc), normals fp32 (B, Hc, Wc, 3), depth fp32 (B, Hc, Wc) -- all of one B, Hc, Wc; ``size`` int32 (B, 2),
    ``coef`` int64 (B, 6), ``side`` fp32 (B, 3) and the two (32, 4) weight tables (data.cubic_table) on the device.  Allocates the
    outputs ((B, Ho, Wo[, 3]) in the source's dtype, returned in job order); ``renormalize=False`` leaves the normals as the
    interpolation and the in-plane rotation give them.  One launch, no host sync."""
    jobs = list(jobs)
    srcs = [s for _, s in jobs]
    L.require_gpu(*srcs, size, coef, side, cubic_q15, cubic_f32)
    if not jobs:
        raise RuntimeError("mtlora_amd: augment_batch needs at least one job")
    B, Hc, Wc = srcs[0].shape[:3]
    Ho, Wo = int(out_size[0]), int(out_size[1])
    for name, t, dt, shape in (("size", size, torch.int32, (B, 2)), ("coef", coef, torch.int64, (B, 6)), ("side", side, torch.float32, (B, 3)),
                               ("cubic_q15", cubic_q15, torch.int32, (32, 4)), ("cubic_f32", cubic_f32, torch.float32, (32, 4))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise RuntimeError(f"mtlora_amd: {name} must be a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    arr = (L.AugmentJob * max(len(jobs), 1))()
    outs = []
    for i, (kind, src) in enumerate(jobs):
        if kind not in AUGMENT_KINDS:
            raise RuntimeError(f"mtlora_amd: unknown augment kind {kind!r}")
        dt, C = _AUGMENT_FORM[kind]
        want = (B, Hc, Wc, 3) if C == 3 else (B, Hc, Wc)
        if src.dtype != dt or tuple(src.shape) != want or not src.is_contiguous():
            raise RuntimeError(f"mtlora_amd: augment job {i} ({kind}) must be a contiguous {dt} tensor of shape {want}, got "
                               f"{src.dtype} {tuple(src.shape)}")
        out = torch.empty((B, Ho, Wo, 3) if C == 3 else (B, Ho, Wo), dtype=dt, device=src.device)
        outs.append(out)
        arr[i].src, arr[i].dst, arr[i].kind = src.data_ptr(), out.data_ptr(), AUGMENT_KINDS[kind]
        arr[i].flags = 0 if renormalize else L.AUGMENT_FLAG_NO_RENORM
    st = L.lib().mtlora_augment_batch(arr, len(jobs), B, Hc, Wc, Ho, Wo, L.ptr(size), L.ptr(coef), L.ptr(side), L.ptr(cubic_q15),
                                      L.ptr(cubic_f32), L.stream_ptr())
    L.check(st, "mtlora_augment_batch")
    return outs


# ----------------------------------------------------------------------------------------------
# plain (library) GEMM linears with a huge row count: weight gradient as a batched GEMM over row chunks
# ----------------------------------------------------------------------------------------------
def _layout_weight(weight, bias, cdtype, col_index, n_cols, pad_rows):
    """the weight as the kernel takes it: ``col_index`` scatters its columns into ``n_cols`` (zero elsewhere: the padded channel
    layout of ConcatUpsampleFn), ``pad_rows`` appends zero rows (classes padded to a multiple of 8).  BigLinearFn hands in DETACHED
    parameters (no autograd nodes for the scatter / cat: ``_unlayout_grads`` is part of its backward), ``linear_big_m`` the parameters.
    (Round 5 also tried the weight / bias gradients of these linears on the factor-gradient side stream -- nothing in the backward
    chain reads them: c2 -0.7 %, c4 -1.0 %, c5:4 -1.0 %: they leave four concurrent task streams for one.  Removed.)"""
    w = weight.to(cdtype)
    if col_index is not None:
        w = w.new_zeros(w.shape[0], n_cols).index_copy(1, col_index, w)
    b = bias
    if pad_rows:
        w = torch.cat([w, w.new_zeros(pad_rows, w.shape[1])], 0)
        b = None if b is None else torch.cat([b, b.new_zeros(pad_rows)], 0)
    return w.contiguous(), b


def _unlayout_grads(dw, db, col_index, pad_rows):
    if pad_rows:
        dw = None if dw is None else dw[:dw.shape[0] - pad_rows]
        db = None if db is None else db[:db.shape[0] - pad_rows].contiguous()
    if col_index is not None and dw is not None:
        dw = dw.index_select(1, col_index)
    elif dw is not None and pad_rows:
        dw = dw.contiguous()
    return dw, db


class BigLinearFn(torch.autograd.Function):
    """y = x W^T + b like F.linear for M = 100k..400k rows, with dW = dY^T X evaluated as a batched GEMM over S row chunks + a sum:
    with an output of a few hundred x a few hundred elements the single GEMM runs on 17-34 workgroups of the 256 CUs (568 us for
    1080x270 over 401k rows), the batched form fills the GPU.  ``weight`` / ``bias`` are the (fp32) master parameters: they are
    cast to ``cdtype`` inside (no autograd cast nodes) and their gradients are returned in the masters' dtype straight from the
    fp32 chunk sum (no bf16 round trip).
    ``via_knt``: forward and dX through the library's fused-GEMM kernel used at rank 0 (``mtlora_linear_fwd/bwd`` with r_s = 0,
    T = 0) instead of hipBLASLt: for the skinny-K / huge-M GEMMs of the heads (e.g. 100k x 272 -> 1080) hipBLASLt reaches ~1.3 TB/s
    and ~12 % of the MFMA peak, k_nt ~3 TB/s (W^T re-materialised per step: the weight is trained); a narrow dW (N <= 64) then
    comes from the library's split-M TN reduction."""

    @staticmethod
    def forward(ctx, x, weight, bias, splits: int, zero_bias_grad: bool, cdtype, via_knt: bool, col_index=None, n_cols=0, pad_rows=0):
        w, bl = _layout_weight(weight.detach(), None if bias is None else bias.detach(), cdtype, col_index, n_cols, pad_rows)
        ctx.wlayout = (col_index, pad_rows)
        ctx.via_knt, ctx.splits, ctx.zero_bias_grad = via_knt, splits, zero_bias_grad
        ctx.has_bias, ctx.wdtype = bias is not None, weight.dtype
        ctx.bdtype = None if bias is None else bias.dtype
        if not via_knt:
            ctx.save_for_backward(x, w)
            return torch.nn.functional.linear(x, w, None if bl is None else bl.to(cdtype))
        L.require_gpu(x, weight)
        M, K = x.shape
        N = w.shape[0]
        ctx.meta = meta = LinearMeta(K=K, N=N, r_s=0, r_t=(), scale_s=0.0, scale_t=(), mode=0, has_x_tasks=False, dropout_p=0.0,
                                     seed=0, dtype=cdtype)
        d = meta.desc(M)
        lib = L.lib()
        ctx_bytes = _size_query("ctx", lib.mtlora_linear_ctx_bytes, d)
        ctxbuf = _scratch(ctx_bytes, x.device, "plain-linear shape (M, K, N)", M, K, N, floor=16)
        y = torch.empty((M, N), dtype=cdtype, device=x.device)
        bf = None if bl is None else bl.float().contiguous()
        st = lib.mtlora_linear_fwd(ctypes.byref(d), L.ptr(x), L.ptr_array(None), L.ptr(w), L.ptr(bf), L.ptr(None), L.ptr(None),
                                   L.ptr_array(None), L.ptr_array(None), L.ptr(y), L.ptr_array(None), L.ptr(ctxbuf), ctx_bytes,
                                   L.stream_ptr())
        L.check(st, "mtlora_linear_fwd (rank 0)")
        ctx.save_for_backward(x, w, ctxbuf)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, *ctxbuf = ctx.saved_tensors
        gy = gy.contiguous()
        M, K = x.shape
        N = w.shape[0]
        S = ctx.splits
        need = ctx.needs_input_grad
        dx = None
        if need[0] and not ctx.via_knt:
            dx = gy @ w
        elif need[0]:
            d = ctx.meta.desc(M)
            lib = L.lib()
            sb = _size_query("bwd", lib.mtlora_linear_bwd_scratch_bytes, d)
            scratch = _scratch(sb, x.device, "plain-linear backward shape (M, K, N)", M, K, N, floor=16)
            wt = w.t().contiguous()
            dx = torch.empty((M, K), dtype=x.dtype, device=x.device)
            st = lib.mtlora_linear_bwd(ctypes.byref(d), L.ptr(x), L.ptr_array(None), L.ptr(wt), L.ptr(gy), L.ptr_array(None),
                                       L.ptr(ctxbuf[0]), ctxbuf[0].numel(), L.ptr(dx), L.ptr_array(None), L.ptr(None), L.ptr(None),
                                       L.ptr_array(None), L.ptr_array(None), L.ptr(scratch), sb, L.stream_ptr())
            L.check(st, "mtlora_linear_bwd (rank 0)")
        dw = None
        if need[1]:
            if ctx.via_knt and N <= 64:  # narrow output: the library's split-M TN reduction reads x once (hipBLASLt: 0.8 TB/s here)
                dw = gemm_tn(gy, x).to(ctx.wdtype)
            else:
                part = torch.bmm(gy.view(S, M // S, N).transpose(1, 2), x.view(S, M // S, K))  # (S, N, K)
                dw = part.sum(0, dtype=torch.float32).to(ctx.wdtype)
        db = None
        if ctx.has_bias and need[2]:
            # zero_bias_grad: the output feeds a training-mode BatchNorm, whose backward returns columns that sum to zero
            # EXACTLY (dx = scale (dy' - mean(dy') - xhat mean(dy' xhat)), sum(xhat) = 0): the bias gradient is 0, and
            # summing 400k x 1080 elements only to obtain rounding noise costs a full pass over the gradient
            if ctx.zero_bias_grad:
                db = torch.zeros(N, dtype=ctx.bdtype, device=gy.device)
            else:  # two-stage column sum: a (400k x 21) sum(0) runs on 64 workgroups for 256 us in one stage
                db = column_sum(gy).to(ctx.bdtype)
        dw, db = _unlayout_grads(dw, db, *ctx.wlayout)
        return dx, dw, db, None, None, None, None, None, None, None


def gemm_tn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(Na, Nb) fp32 = a^T b for row-major (M, Na), (M, Nb) bf16 / fp32 matrices (``mtlora_gemm_tn``)."""
    L.require_gpu(a, b)
    if a.dtype != b.dtype or a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("gemm_tn: (M, Na) and (M, Nb) matrices of one dtype expected")
    a, b = a.contiguous(), b.contiguous()
    M, Na = a.shape
    Nb = b.shape[1]
    lib = L.lib()
    sb = lib.mtlora_gemm_tn_scratch_bytes(M, Na, Nb)
    scratch = _scratch(sb, a.device, "gemm_tn shape (M, Na, Nb)", M, Na, Nb)
    out = torch.empty((Na, Nb), dtype=torch.float32, device=a.device)
    st = lib.mtlora_gemm_tn(L.ptr(a), L.ptr(b), L.ptr(out), M, Na, Nb, Na, Nb, L._DT[a.dtype],
                            L.ptr(scratch), sb, L.stream_ptr())
    L.check(st, "mtlora_gemm_tn")
    return out


_PLAIN_VIA_KNT = os.environ.get("MTLORA_HEAD_GEMM", "knt") != "blas"


def _big_linear(x, weight, bias, S, feeds_batchnorm, cdtype, col_index=None, pad_rows=0):
    K, N = x.shape[1], weight.shape[0] + pad_rows
    via_knt = _PLAIN_VIA_KNT and cdtype in _HOT_DTYPES and K % 8 == 0 and N % 8 == 0 and x.dtype == cdtype
    return BigLinearFn.apply(x, weight, bias, S, feeds_batchnorm, cdtype, via_knt, col_index, K, pad_rows)


def linear_big_m(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                 feeds_batchnorm: bool = False, col_index: Optional[torch.Tensor] = None, pad_rows: int = 0) -> torch.Tensor:
    """F.linear for (M, K) inputs through BigLinearFn when the weight is trained (else plain F.linear).
    feeds_batchnorm=True: the output goes straight into a training-mode BatchNorm -> the bias gradient is exactly 0.
    col_index: x has MORE columns than the weight -- column c of the weight multiplies column col_index[c] of x (the padded channel
    layout of ConcatUpsampleFn; the other columns of x meet zeros).  pad_rows: the output gets that many extra all-zero columns."""
    M = x.shape[0]
    if x.dim() == 2 and x.is_cuda and weight.requires_grad and torch.is_grad_enabled() and M >= 1 and x.is_contiguous():
        S = 1  # small M: one chunk -- still this Function, so that the bias gradient is ``column_sum`` (ATen's sum(0) of a mid-size
               # gradient is a multi-block reduce with a device memset, which a HIP-graph capture of the step cannot replay)
        if M >= 16384:
            # enough row chunks that chunks x output tiles (64 x 64) fills the 256 CUs ~8 times (measured on the heads' 1080 x 272
            # gradient: 235 us at 8 chunks, 114 us at 32), each chunk >= 1024 rows
            tiles = ((weight.shape[0] + 63) // 64) * ((weight.shape[1] + 63) // 64)
            S = 4
            while S < 64 and S * tiles < 2048 and M % (2 * S) == 0 and M // (2 * S) >= 1024:
                S *= 2
            if M % S:
                S = 1
        if torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            with torch.autocast("cuda", enabled=False):
                return _big_linear(x.to(dt), weight, bias, S, feeds_batchnorm, dt, col_index, pad_rows)
        return _big_linear(x, weight, bias, S, feeds_batchnorm, x.dtype, col_index, pad_rows)
    if col_index is not None or pad_rows:
        weight, bias = _layout_weight(weight, bias, weight.dtype, col_index, x.shape[1], pad_rows)
    return torch.nn.functional.linear(x, weight, bias)


# ----------------------------------------------------------------------------------------------
# HRNet head input: [finest map | upsampled coarse maps] concatenated along channels, without the copies
# ----------------------------------------------------------------------------------------------
def _pad4(c: int) -> int:
    return (c + 3) // 4 * 4


class ConcatUpsampleFn(torch.autograd.Function):
    """maps[i]: (B, h_i, w_i, C_i) channels-last, h_0 = H the finest, H = s_i * h_i.  Returns the (B*H*W, ld) matrix
    [maps[0] | pad | up(maps[1]) | up(maps[2]) | ...] (bilinear, align_corners=False) whose slices start at multiples of
    4 channels (``ConcatUpsampleFn.layout(channels)`` gives offsets and ld): the upsample kernels write / read the slices
    of the concatenated matrix directly (csrc/upsample.hip), replacing F.interpolate x3 + torch.cat and their backward."""

    @staticmethod
    def layout(channels):
        offs, o = [], 0
        for c in channels:
            offs.append(o)
            o += _pad4(c)
        return offs, (o + 7) // 8 * 8

    @staticmethod
    def forward(ctx, *maps):
        L.require_gpu(*maps)
        B, H, W, _ = maps[0].shape
        chans = [m.shape[3] for m in maps]
        offs, ld = ConcatUpsampleFn.layout(chans)
        dt = maps[0].dtype
        out = torch.empty(B * H * W, ld, dtype=dt, device=maps[0].device)
        o3 = out.view(B, H, W, ld)
        o3[..., :chans[0]].copy_(maps[0])
        lib = L.lib()
        end = chans[0]
        for i in range(1, len(maps)):
            if offs[i] > end:
                o3[..., end:offs[i]].zero_()
            m = maps[i].contiguous()
            _, h, w, C = m.shape
            if H % h or W % w or H // h != W // w or C % 4 or m.dtype != dt:
                raise RuntimeError("mtlora_amd: ConcatUpsampleFn needs integer scales, C % 4 == 0 and one dtype")
            st = lib.mtlora_upsample_cl_fwd(L.ptr(m), ctypes.c_void_p(out.data_ptr() + offs[i] * out.element_size()), B, h, w, C,
                                            H // h, ld, L.dtype_code(m), L.stream_ptr())
            L.check(st, "mtlora_upsample_cl_fwd")
            end = offs[i] + C
        if ld > end:
            o3[..., end:].zero_()
        ctx.shapes = [tuple(m.shape) for m in maps]
        ctx.offs, ctx.ld = offs, ld
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, H, W, C0 = ctx.shapes[0]
        ld = ctx.ld
        grads = [g.view(B, H, W, ld)[..., :C0]]
        lib = L.lib()
        for i in range(1, len(ctx.shapes)):
            _, h, w, C = ctx.shapes[i]
            d = torch.empty(ctx.shapes[i], dtype=g.dtype, device=g.device)
            st = lib.mtlora_upsample_cl_bwd(ctypes.c_void_p(g.data_ptr() + ctx.offs[i] * g.element_size()), L.ptr(d), B, h, w, C,
                                            H // h, ld, L.dtype_code(g), L.stream_ptr())
            L.check(st, "mtlora_upsample_cl_bwd")
            grads.append(d)
        return tuple(grads)


# ----------------------------------------------------------------------------------------------
# a run of SwinTransformerBlocks without task outputs: ONE autograd node, one library call per block and direction
# (mtlora_block_fwd / mtlora_block_bwd, ABI v7)
# ----------------------------------------------------------------------------------------------
class BlockCall:
    """what one block of a ``SwinBlockRunFn`` call needs besides its tensors: the four linears' metas (seeds drawn, packed factors
    looked up), their frozen-weight copies, the attention geometry.  Built per call by ``SwinTransformerBlock._block_call``."""
    __slots__ = ("has_norm1", "metas", "weights", "mask", "mask_ids", "H", "W", "num_heads", "window_size", "shift", "hidden",
                 "eps", "attn_scale", "mask_value", "factor_params", "norm_params", "desc", "params", "n_flat", "flat_at", "bias_params")

    def __init__(self, has_norm1, metas, weights, mask, mask_ids, H, W, num_heads, window_size, shift, hidden, eps, attn_scale,
                 factor_params, norm_params=(), mask_value=-100.0):
        self.has_norm1, self.metas, self.weights, self.mask, self.mask_ids = has_norm1, metas, weights, mask, mask_ids
        self.H, self.W, self.num_heads, self.window_size, self.shift, self.hidden = H, W, num_heads, window_size, shift, hidden
        self.eps, self.attn_scale, self.mask_value, self.factor_params = eps, attn_scale, mask_value, factor_params
        self.norm_params = tuple(norm_params)
        self.desc = self.params = None
        self.n_flat = 21 if has_norm1 else 19

    def build_desc(self, B: int, C: int, cdtype: torch.dtype, x_dtype: torch.dtype) -> "L.BlockDesc":
        d = L.BlockDesc()
        d.B, d.H, d.W, d.C, d.hidden = B, self.H, self.W, C, self.hidden
        d.num_heads, d.window_size, d.shift = self.num_heads, self.window_size, self.shift
        d.dtype, d.x_dtype, d.has_norm1 = L._DT[cdtype], L._DT[x_dtype], 1 if self.has_norm1 else 0
        d.eps1, d.eps2, d.eps_next = self.eps
        d.attn_scale, d.mask_value = self.attn_scale, self.mask_value
        M = B * self.H * self.W
        for i, m in enumerate(self.metas):
            d.lin[i] = m.desc(M)
        self.desc = d
        return d


_blk_bytes_cache: dict = {}


def _block_bytes(call: "BlockCall", d, B: int, C: int) -> Tuple[int, int, int]:
    """(save, fwd tmp, bwd scratch) bytes of a block call -- three host calls into the library per new geometry"""
    key = (B, call.H, call.W, C, call.hidden, call.has_norm1, d.dtype, d.x_dtype, call.window_size, call.num_heads, call.shift,
           call.mask_ids is not None, tuple((m.r_s, m.packed is not None) for m in call.metas))
    v = _blk_bytes_cache.get(key)
    if v is None:
        lib = L.lib()
        v = (lib.mtlora_block_save_bytes(ctypes.byref(d)), lib.mtlora_block_fwd_tmp_bytes(ctypes.byref(d)),
             lib.mtlora_block_bwd_scratch_bytes(ctypes.byref(d)))
        if min(v) < 0:
            raise RuntimeError(f"mtlora_amd: invalid SwinTransformerBlock geometry B={B} H={call.H} W={call.W} C={C} hidden={call.hidden}")
        _blk_bytes_cache[key] = v
    return v


class SwinBlockRunFn(torch.autograd.Function):
    """(x_out, normed_out) of a run of n consecutive SwinTransformerBlocks WITHOUT task outputs (reference
    swin_transformer_mtlora.py:326-408, tasks-free path): each block is ONE library call forward and ONE (or phase 1 + phase 2 with the
    factor-gradient side stream) backward; the block calls issue exactly the launches of the per-layer Functions above.

    args: calls (list of BlockCall), x (B, L, C) residual stream, normed (norm1(x) of the first block, or None when that block
    applies it itself), then per block
        bias (nH, N, N) fp32, scale1, scale2 ((B) fp32 DropPath factors or None), [norm1.weight, norm1.bias when has_norm1],
        norm2.weight, norm2.bias, next_norm.weight, next_norm.bias, A_qkv, B_qkv, A_proj, B_proj, A_fc1, B_fc1, A_fc2, B_fc2,
        then the four `linear.bias` masters that train with W frozen (None where the bias is frozen or absent): the block call reads
        them as its bias operands and returns their gradients (``mtlora_block_grads.dlin_bias``)"""

    @staticmethod
    def forward(ctx, calls, x, normed, *flat):
        L.require_gpu(x, normed)
        lib = L.lib()
        B, _, C = x.shape
        M = x.numel() // C
        cdtype = calls[0].metas[0].dtype
        if not x.is_contiguous() or (normed is not None and (normed.dtype != cdtype or not normed.is_contiguous())):
            raise RuntimeError("mtlora_amd: SwinBlockRunFn needs contiguous inputs, norm1(x) in the compute dtype")
        stream = L.stream_ptr()
        dev = x.device
        tmp = None
        at = 0
        xs, ns, saves = [x], [normed], []
        for c in calls:
            t = flat[at:at + c.n_flat]
            c.flat_at = at
            c.bias_params = tuple(q for q in t[c.n_flat - 4:] if q is not None)
            at += c.n_flat
            # every tensor whose raw address goes into BlockParams: on x's device, contiguous, in the dtype the kernels read it as
            # (the per-layer Functions report a mismatch as an error; here it would be an illegal access)
            for q in t:
                if q is not None and (q.device != dev or q.dtype != torch.float32 or not q.is_contiguous()):
                    raise RuntimeError("mtlora_amd: SwinBlockRunFn needs contiguous fp32 bias / DropPath / LayerNorm / factor tensors on the input's device")
            for wc, wt, bf in c.weights:
                if (wc.device != dev or wt.device != dev or wc.dtype != cdtype or wt.dtype != cdtype or not wc.is_contiguous()
                        or not wt.is_contiguous() or (bf is not None and (bf.device != dev or bf.dtype != torch.float32 or not bf.is_contiguous()))):
                    raise RuntimeError("mtlora_amd: SwinBlockRunFn needs the frozen-weight copies in the compute dtype on the input's device")
            if c.mask_ids is not None and (c.mask_ids.device != dev or c.mask_ids.dtype != torch.int32 or not c.mask_ids.is_contiguous()):
                raise RuntimeError("mtlora_amd: SwinBlockRunFn needs a contiguous int32 region-id map on the input's device")
            if c.mask is not None and c.mask_ids is None and (c.mask.device != dev or c.mask.dtype != torch.float32 or not c.mask.is_contiguous()):
                raise RuntimeError("mtlora_amd: SwinBlockRunFn needs a contiguous fp32 attention mask on the input's device")
            d = c.build_desc(B, C, cdtype, x.dtype)
            sb, tb, _ = _block_bytes(c, d, B, C)
            p = L.BlockParams()
            k = 3
            p.attn_bias, p.scale1, p.scale2 = t[0].data_ptr(), (0 if t[1] is None else t[1].data_ptr()), (0 if t[2] is None else t[2].data_ptr())
            if c.has_norm1:
                p.norm1_g, p.norm1_b = t[3].data_ptr(), t[4].data_ptr()
                k = 5
            p.norm2_g, p.norm2_b, p.next_g, p.next_b = t[k].data_ptr(), t[k + 1].data_ptr(), t[k + 2].data_ptr(), t[k + 3].data_ptr()
            for i in range(4):
                wc, wt, bf = c.weights[i]
                p.W[i], p.Wt[i], p.bias[i] = wc.data_ptr(), wt.data_ptr(), (0 if bf is None else bf.data_ptr())
                p.A[i], p.Bf[i] = t[k + 4 + 2 * i].data_ptr(), t[k + 5 + 2 * i].data_ptr()
                if t[k + 12 + i] is not None:  # a trainable bias: the operand is the master itself
                    if t[k + 12 + i].numel() != c.metas[i].N:
                        raise RuntimeError("mtlora_amd: SwinBlockRunFn got a bias master that does not match its linear")
                    p.bias[i] = t[k + 12 + i].data_ptr()
            p.mask_ids = 0 if c.mask_ids is None else c.mask_ids.data_ptr()
            p.mask = 0 if (c.mask is None or c.mask_ids is not None) else c.mask.data_ptr()
            c.params = p
            if tmp is None or tmp.numel() < tb:
                tmp = torch.empty(tb, dtype=torch.uint8, device=dev)
            save = torch.empty(sb, dtype=torch.uint8, device=dev)
            x_out = torch.empty_like(xs[-1])
            n_out = torch.empty(x.shape, dtype=cdtype, device=dev)
            st = lib.mtlora_block_fwd(ctypes.byref(d), ctypes.byref(p), xs[-1].data_ptr(), 0 if ns[-1] is None else ns[-1].data_ptr(),
                                      x_out.data_ptr(), n_out.data_ptr(), save.data_ptr(), sb, tmp.data_ptr(), tb, stream)
            L.check(st, "mtlora_block_fwd")
            xs.append(x_out)
            ns.append(n_out)
            saves.append(save)
        n = len(calls)
        ctx.calls, ctx.n, ctx.has_normed = calls, n, normed is not None
        ctx.dims = (B, M, C, cdtype)
        # tensors whose addresses the params structs hold: inputs first (autograd tracks their versions), then the call's own buffers
        ctx.save_for_backward(*xs, *[t for t in ns if t is not None], *saves, *[t for t in flat if t is not None])
        ctx.flat_none = [t is None for t in flat]
        return xs[-1], ns[-1]

    @staticmethod
    def backward(ctx, g_x, g_n):
        calls, n = ctx.calls, ctx.n
        B, M, C, cdtype = ctx.dims
        sv = ctx.saved_tensors
        xs = sv[:n + 1]
        k = n + 1
        ns = list(sv[k:k + n + (1 if ctx.has_normed else 0)])
        k += len(ns)
        if not ctx.has_normed:
            ns = [None] + ns
        saves = sv[k:k + n]
        dev = xs[0].device
        lib = L.lib()
        g_x = g_x.contiguous() if g_x.dtype == xs[0].dtype else g_x.to(xs[0].dtype).contiguous()
        g_n = g_n.contiguous() if g_n.dtype == cdtype else g_n.to(cdtype).contiguous()
        grads_flat = []
        for bi in range(n - 1, -1, -1):
            c = calls[bi]
            d, p = c.desc, c.params
            _, _, scb = _block_bytes(c, d, B, C)
            scratch = torch.empty(scb, dtype=torch.uint8, device=dev)
            nH, N = c.num_heads, c.window_size * c.window_size
            gx = torch.empty_like(xs[bi])
            gn = None if c.has_norm1 else torch.empty(xs[bi].shape, dtype=cdtype, device=dev)
            lnw = torch.empty((6, C), dtype=torch.float32, device=dev)
            dbias = torch.empty((nH, N, N), dtype=torch.float32, device=dev)
            fg = []
            for i, m in enumerate(c.metas):
                fg.append(torch.empty((m.r_s, m.K), dtype=torch.float32, device=dev))
                fg.append(torch.empty((m.N, m.r_s), dtype=torch.float32, device=dev))
            g = L.BlockGrads()
            g.g_x, g.g_normed = gx.data_ptr(), (0 if gn is None else gn.data_ptr())
            g.d_norm1_g, g.d_norm1_b, g.d_norm2_g, g.d_norm2_b = lnw[0].data_ptr(), lnw[1].data_ptr(), lnw[2].data_ptr(), lnw[3].data_ptr()
            g.d_next_g, g.d_next_b, g.dbias = lnw[4].data_ptr(), lnw[5].data_ptr(), dbias.data_ptr()
            at_b = 3 + c.flat_at + c.n_flat - 4  # (the bias masters close this block's flat arguments: see the class docstring)
            need_b = ctx.needs_input_grad[at_b:at_b + 4]
            db = [torch.empty(m.N, dtype=torch.float32, device=dev) if need_b[i] else None for i, m in enumerate(c.metas)]
            for i in range(4):
                g.dA[i], g.dB[i] = fg[2 * i].data_ptr(), fg[2 * i + 1].data_ptr()
                g.dlin_bias[i] = 0 if db[i] is None else db[i].data_ptr()
            fg_all = fg + [t for t in db if t is not None]
            # everything phase 2 writes on the side stream: the eight factor gradients and the LayerNorm dgamma / dbeta (their
            # second-stage reduces ride along, csrc/internal.h) -- none of their Parameters may have a .grad to accumulate into
            args = (ctypes.byref(d), ctypes.byref(p), xs[bi].data_ptr(), 0 if ns[bi] is None else ns[bi].data_ptr(),
                    xs[bi + 1].data_ptr(), g_x.data_ptr(), g_n.data_ptr(), saves[bi].data_ptr(), saves[bi].numel(), ctypes.byref(g),
                    scratch.data_ptr(), scb)
            _run_factor_phases(c.factor_params + c.norm_params + c.bias_params, fg_all, M, dev, True,
                               lambda phase, sp: L.check(lib.mtlora_block_bwd(*args, phase, sp), "mtlora_block_bwd"),
                               lambda: (xs[bi], xs[bi + 1], saves[bi], scratch, lnw, g_n, *fg_all) + (() if ns[bi] is None else (ns[bi],)))
            blk = [dbias, None, None]
            if c.has_norm1:
                blk += [lnw[0], lnw[1]]
            blk += [lnw[2], lnw[3], lnw[4], lnw[5], *fg, *db]
            grads_flat = blk + grads_flat
            g_x, g_n = gx, gn
        return (None, g_x, g_n if ctx.has_normed else None, *grads_flat)
