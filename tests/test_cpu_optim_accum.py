"""Host side of gradient accumulation inside the fused update (mtlora_adamw_accum_update_dev, mtlora_adamw_accum_layout,
FusedAdamW.clip_and_step(accumulation_steps=), GraphedTrainStep(accumulation_steps=)): the additive exports, their bindings, what
they reject before any launch, and the Python argument checks (pure host calls, no GPU)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()


def test_accum_exports_are_declared_and_bound():
    """the header declares both exports with the parameters the ctypes signatures bind, the library exports them, and the two new
    control words sit in the free part of the control block (behind the step counter, in front of the bias corrections)"""
    from mtlora_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    for name in ("mtlora_adamw_accum_update_dev", "mtlora_adamw_accum_layout"):
        assert name in protos and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    params = [" ".join(p.split()) for p in protos["mtlora_adamw_accum_update_dev"].split(",")]
    res, argtypes = _lib._SIGS["mtlora_adamw_accum_update_dev"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == 20
    # the first sixteen are mtlora_adamw_update_dev's, in its order
    dev_params = [" ".join(p.split()) for p in protos["mtlora_adamw_update_dev"].split(",")]
    assert params[:16] == dev_params[:16] and argtypes[:16] == _lib._SIGS["mtlora_adamw_update_dev"][1][:16]
    assert params[16:] == ["float* acc", "const int64_t* acc_offsets", "int accum_steps", "void* stream"]
    assert argtypes[18] is ctypes.c_int
    assert len(protos["mtlora_adamw_accum_layout"].split(",")) == len(_lib._SIGS["mtlora_adamw_accum_layout"][1]) == 4
    assert f"#define MTLORA_ADAMW_CTRL_MICRO {_lib.ADAMW_CTRL_MICRO}" in _header()
    assert f"#define MTLORA_ADAMW_CTRL_UPDATED {_lib.ADAMW_CTRL_UPDATED}" in _header()
    assert 4 < _lib.ADAMW_CTRL_MICRO < _lib.ADAMW_CTRL_UPDATED < 8
    assert "#define MTLORA_ADAMW_MAX_ACCUM_STEPS (1 << 24)" in _header() and _lib.ADAMW_MAX_ACCUM_STEPS == 1 << 24


def test_abi_version_is_still_12():
    from mtlora_amd import _lib
    assert "#define MTLORA_ABI_VERSION 12" in _header()
    assert _lib.ABI_VERSION == 12 == _lib.lib().mtlora_version()
    assert "#define MTLORA_ADAMW_CTRL_WORDS 64" in _header() and _lib.ADAMW_CTRL_WORDS == 64


def test_accum_layout():
    """slices in tensor order, each rounded up to 4 elements (16 bytes); the offsets array is optional"""
    from mtlora_amd import _lib
    L = _lib.lib()
    sizes = [1, 3, 4095, 4096, 4097, 10000, 0, 5]
    numel = (ctypes.c_int64 * len(sizes))(*sizes)
    offs, total = (ctypes.c_int64 * len(sizes))(), ctypes.c_int64()
    assert L.mtlora_adamw_accum_layout(len(sizes), numel, offs, ctypes.byref(total)) == 0
    want, at = [], 0
    for n in sizes:
        want.append(at)
        at += -(-n // 4) * 4
    assert list(offs) == want and total.value == at
    total2 = ctypes.c_int64()
    assert L.mtlora_adamw_accum_layout(len(sizes), numel, None, ctypes.byref(total2)) == 0 and total2.value == at
    assert L.mtlora_adamw_accum_layout(len(sizes), numel, offs, None) == -4
    assert L.mtlora_adamw_accum_layout(len(sizes), None, offs, ctypes.byref(total)) == -4
    assert L.mtlora_adamw_accum_layout(0, numel, offs, ctypes.byref(total)) < 0


def test_accum_update_rejects_before_any_launch():
    """null table / grads / groups_dev / ctrl / scratch / acc / acc_offsets -> MTLORA_ERR_NULL (-4); n_groups 0 and MAX + 1 ->
    MTLORA_ERR_UNSUPPORTED (-7); accum_steps < 1 or above the maximum -> MTLORA_ERR_SHAPE (-2); short scratch ->
    MTLORA_ERR_WORKSPACE (-5); misaligned acc / acc_offsets -> MTLORA_ERR_ALIGN (-3).  No device is touched: the pointers are
    never dereferenced on the host, and this machine need not have a GPU."""
    from mtlora_amd import _lib
    L = _lib.lib()

    def call(table=16, grads=16, groups=16, n_groups=1, ctrl=16, scratch=16, scratch_bytes=8, acc=16, acc_offsets=16, k=2):
        return L.mtlora_adamw_accum_update_dev(table, grads, 1, 1, groups, n_groups, 0.0, ctrl, None, None, None, 2.0, 0.5, 1, scratch,
                                               scratch_bytes, acc, acc_offsets, k, None)

    for name in ("table", "grads", "groups", "ctrl", "scratch", "acc", "acc_offsets"):
        assert call(**{name: None}) == -4, name
    assert call(n_groups=0) == -7
    assert call(n_groups=_lib.ADAMW_MAX_GROUPS + 1) == -7
    assert call(n_groups=_lib.ADAMW_MAX_GROUPS, scratch_bytes=4) == -5
    for k in (0, -1, _lib.ADAMW_MAX_ACCUM_STEPS + 1):
        assert call(k=k) == -2, k
    assert call(k=1, acc=None) == -4  # (k = 1 never reads acc, and still checks it)
    assert call(groups=20) == -3 and call(acc=20) == -3 and call(acc_offsets=20) == -3
    assert L.mtlora_error_string(-2) and L.mtlora_error_string(-3)


def test_accumulation_steps_argument_checks():
    """k = 0, k = 1.5 (and a bool, a string) raise ValueError; a by-value FusedAdamW asked for k = 2 raises TypeError -- both before
    anything touches a device, so the optimizer here is a bare object with only the attribute the check reads"""
    from mtlora_amd.optim import FusedAdamW, accumulation_steps_of
    assert accumulation_steps_of(1) == 1 and accumulation_steps_of(7) == 7
    for bad in (0, -2, 1.5, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="accumulation_steps"):
            accumulation_steps_of(bad)
    p = inspect.signature(FusedAdamW.clip_and_step).parameters
    assert list(p)[1:] == ["max_norm", "scaler", "accumulation_steps"] and p["accumulation_steps"].default == 1
    assert inspect.signature(FusedAdamW.bump_versions).parameters["updated"].default is True
    opt = FusedAdamW.__new__(FusedAdamW)
    opt._capturable = False
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match="accumulation_steps"):
            opt.clip_and_step(5.0, None, accumulation_steps=bad)
    with pytest.raises(TypeError, match="capturable=True"):
        opt.clip_and_step(5.0, None, accumulation_steps=2)
    with pytest.raises(TypeError, match="capturable=True"):
        opt.prepare_accumulation()


def test_graphed_train_step_argument_checks():
    """GraphedTrainStep: k = 0 / 1.5 -> ValueError; a reducer with k = 2 -> ValueError (no DDP inside the accumulating graph); a
    torch optimizer with k = 2 -> TypeError; all before the model or a device is touched"""
    import torch
    from mtlora_amd import mtl_harness as H
    p = inspect.signature(H.GraphedTrainStep.__init__).parameters
    assert p["accumulation_steps"].default == 1
    img = torch.zeros(1)
    lin = torch.nn.Linear(2, 2)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match="accumulation_steps"):
            H.GraphedTrainStep(None, None, sgd, img, {}, accumulation_steps=bad)
    with pytest.raises(ValueError, match="reducer"):
        H.GraphedTrainStep(None, None, sgd, img, {}, reducer=object(), accumulation_steps=2)
    with pytest.raises(TypeError, match="HIP optimizer"):
        H.GraphedTrainStep(None, None, sgd, img, {}, accumulation_steps=2)
    with pytest.raises(TypeError, match="loss_scaler"):  # unchanged: a scaler with a torch optimizer
        H.GraphedTrainStep(None, None, sgd, img, {}, loss_scaler=object())
