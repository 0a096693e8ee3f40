"""CPU tests of the prediction path (csrc/predict.hip through the C ABI, evaluation.get_output_low,
mtl_harness.predict_step): the symbol, the rejections that must happen before any launch, the failure mode on CPU tensors and
the public signatures.  No GPU needed: every call here returns before it touches a device."""
import inspect

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from mtlora_amd.csrc.build import build
    build(verbose=False)
    from mtlora_amd import _lib
    return _lib.lib()


def _call(L, kind, C, scale, out_dtype, dtype=0):
    return L.mtlora_upsample_predict(kind, None, None, 2, 8, 8, C, scale, dtype, out_dtype, None)


def test_symbol_exported_at_abi_11(lib):
    from mtlora_amd import _lib
    assert "mtlora_upsample_predict" in _lib.EXPORTS
    assert lib.mtlora_version() == _lib.ABI_VERSION >= 11
    assert (_lib.F32, _lib.BF16, _lib.F16, _lib.U8) == (0, 1, 2, 3)


def test_rejections_return_unsupported_without_a_launch(lib):
    """null pointers everywhere: a call that got past the checks would return MTLORA_ERR_NULL (-4), not -7"""
    from mtlora_amd import _lib
    UNSUPPORTED, NULL = -7, -4
    F32, U8 = _lib.F32, _lib.U8
    assert _call(lib, 0, 49, 4, U8) == UNSUPPORTED        # argmax: C <= 48
    assert _call(lib, 1, 5, 4, F32) == UNSUPPORTED        # normals: C <= 4
    assert _call(lib, 2, 2, 4, F32) == UNSUPPORTED        # sigmoid: C = 1
    assert _call(lib, 0, 21, 0, U8) == UNSUPPORTED        # scale 1..32
    assert _call(lib, 0, 21, 33, U8) == UNSUPPORTED
    assert _call(lib, 3, 1, 4, U8) == UNSUPPORTED         # identity is fp32 only
    assert _call(lib, 0, 21, 4, F32) == UNSUPPORTED       # argmax is uint8 only
    assert _call(lib, 1, 3, 4, _lib.BF16) == UNSUPPORTED  # not an output dtype
    assert _call(lib, 4, 1, 4, F32) == UNSUPPORTED        # unknown kinds
    assert _call(lib, -1, 1, 4, F32) == UNSUPPORTED
    # every pair of the table gets past them (and stops at the null pointers), for every input dtype
    for kind, C, od in ((0, 21, U8), (0, 48, U8), (1, 3, F32), (1, 4, U8), (2, 1, F32), (2, 1, U8), (3, 1, F32)):
        for scale in (1, 8, 32):
            for dt in (_lib.F32, _lib.BF16, _lib.F16):
                assert _call(lib, kind, C, scale, od, dt) == NULL, (kind, C, od, scale, dt)
    assert _call(lib, 0, 21, 4, U8, dtype=7) == -1         # MTLORA_ERR_DTYPE
    assert lib.mtlora_upsample_predict(0, None, None, 0, 8, 8, 21, 4, F32, U8, None) == 0  # an empty batch is nothing to do
    assert lib.mtlora_upsample_predict(0, None, None, 2, 0, 8, 21, 4, F32, U8, None) == -2


def test_get_output_low_has_no_cpu_fallback():
    from mtlora_amd import functional as Fn
    from mtlora_amd.evaluation import get_output_low
    for task, C in (("semseg", 21), ("human_parts", 7), ("normals", 3), ("sal", 1), ("edge", 1), ("depth", 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            get_output_low(torch.randn(2, 4, 4, C), task, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.upsample_predict("sigmoid", torch.randn(2, 4, 4, 1), 2, out_dtype=torch.uint8)
    with pytest.raises(ValueError):
        get_output_low(torch.randn(2, 4, 4, 1), "nothing", 2)
    with pytest.raises(RuntimeError, match="unknown fused prediction kind"):
        Fn.upsample_predict("softmax", torch.randn(2, 4, 4, 1), 2)
    assert Fn.PREDICT_KINDS == {"argmax": 0, "normals": 1, "sigmoid": 2, "identity": 3}


def test_public_signatures():
    from mtlora_amd import functional as Fn
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.evaluation import get_output_low
    sig = inspect.signature(H.predict_step)
    assert list(sig.parameters) == ["model", "images", "tasks", "uint8", "amp_dtype"]
    assert sig.parameters["tasks"].default is None and sig.parameters["uint8"].default is False
    assert sig.parameters["amp_dtype"].default is torch.bfloat16
    assert inspect.isgeneratorfunction(H.predict)
    assert list(inspect.signature(H.predict).parameters)[:2] == ["model", "batches"]
    sig = inspect.signature(get_output_low)
    assert list(sig.parameters) == ["low", "task", "scale", "uint8"] and sig.parameters["uint8"].default is False
    sig = inspect.signature(Fn.upsample_predict)
    assert list(sig.parameters) == ["kind", "low", "scale", "out_dtype", "out"]
    assert sig.parameters["out_dtype"].default is None and sig.parameters["out"].default is None


def test_predict_step_restores_training_flag_when_it_raises():
    """a CPU batch cannot be predicted (no fallback); the model's mode must come back all the same"""
    from mtlora_amd import mtl_harness as H

    class Low(torch.nn.Module):
        tasks = ["sal"]

        def forward(self, x, upsample=True):
            return {"sal": torch.zeros(x.shape[0], 4, 4, 1)}

    m = Low().train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.predict_step(m, torch.zeros(2, 3, 8, 8))
    assert m.training
    with pytest.raises(RuntimeError, match="integer scale"):
        H.predict_step(m, torch.zeros(2, 3, 8, 6))
    assert m.training
