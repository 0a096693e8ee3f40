"""Host side of the capturable fused update (mtlora_adamw_update_dev, FusedAdamW(capturable=True)): the additive export, its
binding, and what it rejects before any launch (pure host calls, no GPU)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "mtlora_hip.h")).read()


def test_update_dev_is_declared_and_bound():
    """the header declares mtlora_adamw_update_dev with as many parameters as the ctypes signature that binds it (the mechanism of
    test_header_prototypes_match_ctypes_signatures), doubles where the issue puts them, and the library exports it"""
    import ctypes
    from mtlora_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = dict(re.findall(r"\b(mtlora_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr))
    assert "mtlora_adamw_update_dev" in protos
    params = [" ".join(p.split()) for p in protos["mtlora_adamw_update_dev"].split(",")]
    res, argtypes = _lib._SIGS["mtlora_adamw_update_dev"]
    assert res is ctypes.c_int and len(params) == len(argtypes) == 17
    assert params[4] == "const mtlora_adamw_group* groups_dev"
    assert params[11] == "double growth_factor" and params[12] == "double backoff_factor"
    assert argtypes[11] is ctypes.c_double and argtypes[12] is ctypes.c_double and argtypes[6] is ctypes.c_float
    assert "mtlora_adamw_update_dev" in _lib.EXPORTS
    assert _lib.lib().mtlora_adamw_update_dev is not None
    # the device buffer: MAX_GROUPS records (5 doubles) and, behind them, 8 floats per group that the library derives
    assert f"#define MTLORA_ADAMW_GROUPS_DEV_BYTES {_lib.ADAMW_GROUPS_DEV_BYTES}" in _header()
    assert _lib.ADAMW_GROUPS_DEV_BYTES == _lib.ADAMW_MAX_GROUPS * (ctypes.sizeof(_lib.AdamwGroup) + 32)


def test_abi_version_stays_12():
    from mtlora_amd import _lib
    assert "#define MTLORA_ABI_VERSION 12" in _header()
    assert _lib.ABI_VERSION == 12 == _lib.lib().mtlora_version()
    assert "#define MTLORA_ADAMW_CTRL_WORDS 64" in _header() and _lib.ADAMW_CTRL_WORDS == 64  # the ctrl layout did not move


def test_update_dev_rejects_before_any_launch():
    """null table / grads / groups_dev / ctrl / scratch -> MTLORA_ERR_NULL (-4); n_groups 0 and OPT_MAXG + 1 ->
    MTLORA_ERR_UNSUPPORTED (-7); no device is touched (the pointers are never dereferenced on the host)"""
    from mtlora_amd import _lib
    L = _lib.lib()

    def call(table=16, grads=16, groups=16, n_groups=1, ctrl=16, scratch=16, scratch_bytes=8):
        return L.mtlora_adamw_update_dev(table, grads, 1, 1, groups, n_groups, 0.0, ctrl, None, None, None, 2.0, 0.5, 1, scratch,
                                         scratch_bytes, None)

    for name in ("table", "grads", "groups", "ctrl", "scratch"):
        assert call(**{name: None}) == -4, name
    assert call(n_groups=0) == -7
    assert call(n_groups=_lib.ADAMW_MAX_GROUPS + 1) == -7
    assert call(n_groups=_lib.ADAMW_MAX_GROUPS, scratch_bytes=4) == -5  # (a valid group count gets as far as the workspace check)
    assert call(groups=20) == -3  # the records are doubles: 8-byte aligned


def test_fused_adamw_signature_has_capturable():
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import FusedAdamW
    p = inspect.signature(FusedAdamW.__init__).parameters
    assert "capturable" in p and p["capturable"].default is False
    assert callable(FusedAdamW.push_hyperparameters) and callable(FusedAdamW.bump_versions)
    assert "capturable" in inspect.signature(H.build_optimizer).parameters
    assert "loss_scaler" in inspect.signature(H.GraphedTrainStep.__init__).parameters
