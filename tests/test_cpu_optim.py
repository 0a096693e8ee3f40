"""Host side of the fused clip + loss scaler + AdamW update (mtlora_amd/optim.py, csrc/optim.hip): what is rejected, and the
chunk table of the C ABI (pure host calls, no GPU)."""
import ctypes

import pytest
import torch


def _tiny_model(dtype=torch.float32):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.LayerNorm(8)).to(dtype)


def test_hip_optimizer_on_cpu_parameters_raises():
    from mtlora_amd import mtl_harness as H
    with pytest.raises(RuntimeError, match="must live on a ROCm GPU"):
        H.build_optimizer(_tiny_model(), impl="hip")
    with pytest.raises(ValueError, match="impl"):
        H.build_optimizer(_tiny_model(), impl="triton")
    assert isinstance(H.build_optimizer(_tiny_model()), torch.optim.AdamW)  # the default stays torch's


def test_amsgrad_maximize_and_non_fp32_raise():
    from mtlora_amd.optim import FusedAdamW
    ps = list(_tiny_model().parameters())
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW(ps, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdamW(ps, maximize=True)
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([{"params": ps, "amsgrad": True}])
    with pytest.raises(TypeError, match="fp32 parameters only"):
        FusedAdamW(list(_tiny_model(torch.bfloat16).parameters()))
    with pytest.raises(TypeError, match="fp32 parameters only"):
        FusedAdamW(list(_tiny_model(torch.float16).parameters()))


def test_unequal_steps_raise():
    """FusedAdamW.load_state_dict starts with optim.uniform_step (one device counter for all parameters): a torch AdamW state whose
    per-parameter steps differ is refused before anything is touched.  (The whole load_state_dict needs a GPU: test_gpu_optim.)"""
    from mtlora_amd.optim import uniform_step
    m = _tiny_model()
    ps = list(m.parameters())
    opt = torch.optim.AdamW(ps, lr=1e-2)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    ps[0].grad, ps[1].grad = None, None  # these two stay at step 1
    opt.step()
    sd = opt.state_dict()
    with pytest.raises(ValueError, match="one step counter"):
        uniform_step(sd["state"])
    for s in sd["state"].values():
        s["step"] = torch.tensor(2.0)
    assert uniform_step(sd["state"]) == 2.0
    assert uniform_step({}) == 0.0


def test_loss_scaler_host_side():
    from mtlora_amd.optim import LossScaler
    sc = LossScaler(init_scale=1024.0, growth_interval=2)
    sd = sc.state_dict()
    assert sd == {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2, "_growth_tracker": 0}
    other = LossScaler()
    other.load_state_dict(dict(sd, scale=64.0, _growth_tracker=1))
    assert other.state_dict() == dict(sd, scale=64.0, _growth_tracker=1)
    with pytest.raises(RuntimeError, match="empty"):
        other.load_state_dict({})
    with pytest.raises(ValueError):
        LossScaler(growth_factor=1.0)
    opt = torch.optim.AdamW(_tiny_model().parameters())
    with pytest.raises(TypeError, match="FusedAdamW only"):  # refused before backward runs
        sc(torch.zeros((), requires_grad=True), opt)


def test_train_step_refuses_scaler_without_hip_optimizer():
    from mtlora_amd import mtl_harness as H
    from mtlora_amd.optim import LossScaler
    m = _tiny_model()
    with pytest.raises(TypeError, match="impl='hip'"):
        H.train_step(m, None, H.build_optimizer(m), torch.zeros(1, 8), {}, loss_scaler=LossScaler())


def test_chunk_table_of_the_abi():
    """mtlora_adamw_sizes / mtlora_adamw_table: one chunk per 4096 elements of each tensor, in tensor order; the table is
    [n_tensors] x {p, m, v, numel, group, pad} (40 bytes) then [n_chunks] x {tensor, chunk index}."""
    from mtlora_amd import _lib
    L = _lib.lib()
    numel = [1, 4096, 4097, 0, 3 * 4096 + 5]
    nt = len(numel)
    A = (ctypes.c_int64 * nt)(*numel)
    nc, tb, sb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.mtlora_adamw_sizes(nt, A, ctypes.byref(nc), ctypes.byref(tb), ctypes.byref(sb)) == 0
    assert nc.value == 1 + 1 + 2 + 0 + 4 and tb.value == 40 * nt + 8 * nc.value and sb.value == 8 * nc.value
    PA = ctypes.c_void_p * nt
    p, m, v = PA(*[0x1000 * (i + 1) for i in range(nt)]), PA(*[0x100000 + 64 * i for i in range(nt)]), PA(*[0x200000 + 64 * i for i in range(nt)])
    grp = (ctypes.c_int32 * nt)(0, 1, 0, 1, 15)
    host = torch.zeros(tb.value // 8, dtype=torch.int64)
    assert L.mtlora_adamw_table(nt, A, grp, p, m, v, host.data_ptr(), tb.value) == 0
    te = host[:5 * nt].view(nt, 5)
    assert te[:, 0].tolist() == [0x1000 * (i + 1) for i in range(nt)] and te[:, 3].tolist() == numel
    assert (te[:, 4] & 0xFFFFFFFF).tolist() == [0, 1, 0, 1, 15]
    ce = host[5 * nt:].view(torch.int32).view(-1, 2).tolist()
    assert ce == [[0, 0], [1, 0], [2, 0], [2, 1], [4, 0], [4, 1], [4, 2], [4, 3]]
    # rejected before anything is written or launched
    assert L.mtlora_adamw_table(nt, A, grp, p, m, v, host.data_ptr(), tb.value - 8) == -5
    grp[0] = 16
    assert L.mtlora_adamw_table(nt, A, grp, p, m, v, host.data_ptr(), tb.value) == -2
    grp[0] = 0
    p[1] = 0x1002
    assert L.mtlora_adamw_table(nt, A, grp, p, m, v, host.data_ptr(), tb.value) == -3
    assert L.mtlora_adamw_sizes(0, A, ctypes.byref(nc), ctypes.byref(tb), ctypes.byref(sb)) == -2
    g = (_lib.AdamwGroup * 1)()
    assert L.mtlora_adamw_update(None, None, 1, 1, g, 1, 0.0, None, None, None, None, 2.0, 0.5, 1, None, 0, None) == -4
    assert L.mtlora_adamw_update(16, 16, 1, 1, g, 17, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 8, None) == -7
    assert L.mtlora_adamw_update(16, 16, 1, 1, g, 1, 0.0, 16, None, None, None, 2.0, 0.5, 1, 16, 4, None) == -5
