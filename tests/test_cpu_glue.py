"""Host-only checks of the autograd glue (mtlora_amd/functional.py): the key of the size-query cache."""
import ctypes

import pytest
import torch

from mtlora_amd import _lib as L
from mtlora_amd import functional as Fn


def _desc(**over):
    meta = Fn.LinearMeta(K=96, N=384, r_s=16, r_t=(4, 4), scale_s=2.0, scale_t=(1.5, 1.5), mode=0, has_x_tasks=True, dropout_p=0.1,
                         seed=7, dtype=torch.bfloat16)
    d = meta.desc(3136)
    for k, v in over.items():
        if k == "r_t1":
            d.r_t[1] = v
        else:
            setattr(d, k, v)
    return d


# one changed value per field of the documented superset (functional._size_query): what a size query of the library may depend on
KEY_FIELDS = [("M", 3137), ("K", 192), ("N", 768), ("dtype", L.F32), ("mode", 1), ("T", 1), ("r_s", 8), ("r_t1", 8),
              ("has_x_tasks", 0), ("sel_stream", 1), ("sel_dense", 2), ("sel_tn", 2), ("sel_projk", 3), ("max_cu", 64),
              ("packed", 0x1000), ("hid", L.HID_P_GIVEN)]
# pointers' values and per-call values: they enter no size
FREE_FIELDS = [("seed", 12345), ("bwd_phase", 2), ("seed_offset", 0x2000), ("hid_ptr", 0x3000)]


def _asked_again(second, third=None):
    """does ``_size_query`` call the library again for (second[, third]) after it was asked for the unchanged descriptor(s)?"""
    calls = []

    def fn(*refs):
        calls.append(len(refs))
        return 64

    keep = dict(Fn._size_cache)
    Fn._size_cache.clear()
    try:
        if third is None:
            assert Fn._size_query("probe", fn, _desc()) == 64 and Fn._size_query("probe", fn, second) == 64
        else:
            assert Fn._size_query("probe", fn, _desc(), _desc()) == 64 and Fn._size_query("probe", fn, second, third) == 64
    finally:
        Fn._size_cache.clear()
        Fn._size_cache.update(keep)
    return len(calls) == 2


@pytest.mark.parametrize("field,value", KEY_FIELDS)
def test_size_query_key_sees_every_field_a_query_reads(field, value):
    """the key that ``_size_query`` itself builds, for the one descriptor of a one-descriptor query and for either of two"""
    changed = {field: value}
    assert _asked_again(_desc(**changed)), field
    assert _asked_again(_desc(**changed), _desc()) and _asked_again(_desc(), _desc(**changed)), field


def test_size_query_key_ignores_pointers_and_per_call_values():
    assert not _asked_again(_desc()) and not _asked_again(_desc(), _desc())
    for field, value in FREE_FIELDS:
        changed = {field: value}
        assert not _asked_again(_desc(**changed)), field
        assert not _asked_again(_desc(**changed), _desc()) and not _asked_again(_desc(), _desc(**changed)), field
    # of ``packed`` only whether it is set
    calls = []
    keep = dict(Fn._size_cache)
    try:
        for ptr in (0x1000, 0x7000):
            Fn._size_query("probe_packed", lambda ref: calls.append(1) or 8, _desc(packed=ptr))
    finally:
        Fn._size_cache.clear()
        Fn._size_cache.update(keep)
    assert calls == [1]
    # every field of the descriptor is either in the key or known to be free: a field added to the struct must be sorted into one list
    sorted_in = {f for f, _ in KEY_FIELDS + FREE_FIELDS} | {"r_t", "scale_s", "scale_t", "dropout_p", "hid_pad_"}
    sorted_in.discard("r_t1")
    assert {f[0] for f in L.LinearDesc._fields_} == sorted_in


def test_size_query_asks_once_per_key_and_per_query():
    calls = []

    def one(dref):
        calls.append("one")
        return 100

    def two(dref, dref2):
        calls.append("two")
        return 200

    keep = dict(Fn._size_cache)
    try:
        assert Fn._size_query("one", one, _desc()) == 100 and Fn._size_query("one", one, _desc(seed=9)) == 100
        assert Fn._size_query("two", two, _desc(), _desc()) == 200 and Fn._size_query("two", two, _desc(), _desc(bwd_phase=1)) == 200
        assert calls == ["one", "two"]
        assert Fn._size_query("two", two, _desc(), _desc(max_cu=8)) == 200 and Fn._size_query("one", one, _desc(M=64)) == 100
        assert calls == ["one", "two", "two", "one"]
    finally:
        Fn._size_cache.clear()
        Fn._size_cache.update(keep)


def test_scratch_refuses_a_negative_size():
    with pytest.raises(RuntimeError, match=r"invalid gemm_tn shape \(M, Na, Nb\) \(5, 3, 2\)"):
        Fn._scratch(-1, "cpu", "gemm_tn shape (M, Na, Nb)", 5, 3, 2)
    assert Fn._scratch(0, "cpu", "x").numel() == 0 and Fn._scratch(0, "cpu", "x", floor=16).numel() == 16
    assert Fn._scratch(40, "cpu", "x", floor=16).dtype == torch.uint8 and Fn._scratch(40, "cpu", "x", floor=16).numel() == 40
    assert ctypes.sizeof(L.LinearDesc) == len(bytes(_desc()))
