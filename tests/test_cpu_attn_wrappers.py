"""The attention wrappers refuse, in Python, views the kernels would index wrongly (no GPU needed: the checks run before the
library is touched; tests/test_gpu_attn_routes.py checks that nothing is launched on the device)."""
import pytest
import torch

from ultrasound_modeling_amd import ops

B, N, NH = 2, 40, 2
HS = 128 * NH


def z(*s, dt=torch.bfloat16):
    return torch.zeros(*s, dtype=dt)


@pytest.mark.parametrize("which", ["lse_transposed", "lse_short", "out32_bf16", "out32_strided"])
def test_flash_fwd_refuses(which):
    qkv, out = z(B, N, 1, 3 * HS), z(B, N, 1, HS)
    lse, o32 = z(B * NH, N, dt=torch.float32), z(B, N, HS, dt=torch.float32)
    bad = {"lse_transposed": (z(N, B * NH, dt=torch.float32).T, o32), "lse_short": (z(B * NH, N - 1, dt=torch.float32), o32),
           "out32_bf16": (lse, z(B, N, HS)), "out32_strided": (lse, z(B, N, HS + 8, dt=torch.float32)[..., :HS])}[which]
    with pytest.raises(AssertionError, match="lse|out32"):
        ops.flash_attn_fwd(qkv, NH, 1.0, out, *bad)


@pytest.mark.parametrize("which", ["delta_f64", "delta_long", "lse_transposed", "out32_strided"])
def test_flash_bwd_refuses(which):
    qkv, out, d_out, dqkv = z(B, N, 1, 3 * HS), z(B, N, 1, HS), z(B, N, 1, HS), z(B, N, 1, 3 * HS)
    lse, delta, o32 = z(B * NH, N, dt=torch.float32), z(B * NH, N, dt=torch.float32), z(B, N, HS, dt=torch.float32)
    args = {"delta_f64": (lse, z(B * NH, N, dt=torch.float64), o32), "delta_long": (lse, z(B * NH, N + 1, dt=torch.float32), o32),
            "lse_transposed": (z(N, B * NH, dt=torch.float32).T, delta, o32),
            "out32_strided": (lse, delta, z(B, N, HS + 8, dt=torch.float32)[..., :HS])}[which]
    lse_, delta_, o32_ = args
    with pytest.raises(AssertionError, match="lse|delta|out32"):
        ops.flash_attn_bwd(qkv, NH, 1.0, out, d_out, lse_, delta_, dqkv, o32_)


def test_window_bwd_refuses_dqkv_without_qkv_row_stride():
    C, heads = 64, 2
    qv = z(1, 8, 8, 3 * C + 16)[..., 8:8 + 3 * C]
    table = z(49, heads, dt=torch.float32)
    with pytest.raises(AssertionError, match="row stride"):
        ops.window_attn_bwd(qv, z(1, 8, 8, C), table, heads, 4, 0, z(1, 8, 8, 3 * C), torch.zeros_like(table))
    with pytest.raises(AssertionError, match="row stride"):
        ops.window_attn_bwd(z(1, 8, 8, 3 * C), z(1, 8, 8, C), table, heads, 4, 0, qv, torch.zeros_like(table))
