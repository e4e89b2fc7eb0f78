"""Per-kernel parity tests (GPU): every C-ABI kernel against the fp64 CPU oracle on the same seeded inputs.

Tolerance (stated once, used everywhere): inputs and weights are made exactly bf16-representable, the oracle runs
in fp64 on those same values, and
  * fp32 kernel outputs must match within REL_F32 = 1e-3 relative L2 (they land near 1e-6),
  * bf16 kernel outputs must match the oracle ROUNDED TO bf16 within REL_BF16 = 1e-3 relative L2
    (an exact kernel differs from the rounded oracle only where fp32 accumulation order flips a rounding).
"""
import math

import pytest
import torch

import usseg_oracle as O
from route_probe import U_BF16, U_F32, assert_elementwise, c_f32, check, check_norm_bwd, kernels, kname, ng_of, norm_ref, sa_reference, short

pytestmark = pytest.mark.gpu

REL_F32 = 1e-3
REL_BF16 = 1e-3
DEV = "cuda"


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def rnd(gen, *shape, scale=1.0):
    return bf(torch.randn(*shape, generator=gen, dtype=torch.float64) * scale)


def to_dev_padded(x64, cp=None):
    """fp64 NHWC [B,H,W,C] (bf16-representable) -> device bf16 [B,H,W,roundup(C,8)] with zero pads."""
    B, H, W, C = x64.shape
    cp = cp or (C + 7) // 8 * 8
    out = torch.zeros(B, H, W, cp, dtype=torch.bfloat16)
    out[..., :C] = x64.to(torch.bfloat16)
    return out.to(DEV)


def finalize(layer):
    from ultrasound_modeling_amd.flat import FlatParams
    return FlatParams(layer, DEV)


def on_route(want, fn):
    """fn() after asserting the device kernels it launched include `want` (a short kernel name, or a tuple of them): the route a
    case's label names is checked before any of its numbers."""
    out, got = kernels(fn)
    got = [short(n) for n in got]
    for w in (want,) if isinstance(want, str) else want:
        assert w in got, f"expected kernel {w!r}, launched {got}"
    return out


@pytest.fixture(scope="module")
def gen():
    return torch.Generator().manual_seed(1234)


# ------------------------------------------------------------------------------------------------ Conv2D
CONV_CASES = [
    # B, H, W, Cin, Cout, k, dil
    (2, 8, 8, 8, 8, 3, 1),
    (1, 5, 7, 1, 16, 3, 1),       # stem conv1 shape class: Cin 1 -> pad 8, ragged spatial size
    (2, 16, 16, 16, 32, 3, 1),
    (1, 12, 20, 32, 32, 3, 1),
    (2, 9, 11, 30, 64, 3, 1),     # concats_2 stage 1 (Cin 30 -> pad 32)
    (1, 16, 16, 63, 128, 3, 1),   # concats_2 stage 2, Cout > 64 -> BN=128 tile
    (3, 7, 5, 40, 24, 1, 1),      # 1x1, odd everything
    (1, 32, 32, 64, 16, 3, 2),    # dilated branches
    (1, 24, 24, 128, 16, 3, 4),
    (1, 20, 20, 72, 136, 3, 8),   # dilation larger than half the image, Cout spans two N tiles
    (1, 1, 1, 10, 5, 1, 1),       # dense on a [B,1,1,C] tensor
    # lattice classes of the LDS-DMA kernel (conv_big.hip): Cin > 32, lattice width 16 / 8 / 4, ragged channel tails, partial groups.
    # At these sizes (< 128 workgroups) the planner sends the forward passes to conv_halo (8x16 lattice: conv_stream) and only the
    # 256-channel backward-data pass to conv_big; the last case reaches conv_big on the forward pass (CONV_ROUTES)
    (2, 16, 16, 72, 136, 3, 2),   # 8x8 lattices (4 per workgroup), Cin tail 72 = 2*32 + 8, three N tiles (last partial)
    (3, 16, 16, 96, 40, 3, 4),    # 4x4 lattices (16 per workgroup)
    (1, 32, 16, 40, 64, 3, 1),    # two 16x16 patches, second channel chunk partial
    (5, 8, 8, 64, 24, 3, 1),      # 5 patches -> last workgroup has one valid patch of four
    (1, 8, 16, 64, 32, 3, 1),     # one 8x16 patch in a two-patch workgroup
    (2, 32, 32, 256, 64, 3, 1),   # eight channel chunks through the double buffer
    (1, 128, 128, 64, 64, 3, 1),  # 128 workgroups of 128 pixels, 73 KB of weights (too many for conv_stream): conv_big forward
    # halo-tile kernel variants (conv_halo.hip): lattice patches 8x16, 8x8 (2 per workgroup), 4x4 (8 per workgroup), 4x8.
    # The out_f32 pass of every case runs conv_halo; the bf16 passes of the cases with 16-wide lattices and <= 40 KB of weights
    # run conv_stream (stream_plan) - CONV_ROUTES lists each pass
    (2, 32, 32, 64, 64, 3, 8),    # d=8 on 32x32: 4x4 virtual images
    (1, 32, 32, 48, 24, 3, 4),    # d=4 on 32x32: 8x8 virtual images, Cin not a multiple of 32
    (1, 64, 32, 88, 16, 3, 2),    # d=2: 32x16 lattice, Cin = 88 (cardinal conv2 input width at stage 4)
    (3, 16, 16, 24, 136, 3, 1),   # N spans several channel tiles, 3 images -> ragged last workgroup
    (1, 64, 64, 8, 16, 3, 1),     # stem conv1 class
    (2, 16, 32, 32, 8, 3, 4),     # 4x8 lattice patches (4 per workgroup)
    (5, 8, 8, 16, 32, 3, 1),      # 8x8 images, odd batch: last workgroup half empty
    # persistent-weights variant (>= 1024 pixel groups, whole weight operand resident in LDS).  conv_stream takes the bf16 passes
    # of the first three (16-wide lattices); they reach conv_halo_persist on the out_f32 pass only, and the decoder b2 class not at
    # all (its out_f32 pass is a conv_big launch).  The last case (8-wide lattice) reaches it on every pass
    (2, 256, 256, 16, 32, 3, 1),  # stem convtmp_1 class, 1024 groups
    (2, 256, 256, 64, 16, 3, 4),  # decoder b2 class: 2 channel chunks resident, dilation 4
    (5, 256, 128, 24, 8, 3, 2),   # 1280 groups, 2 per workgroup, Cin not a multiple of 32
    (8, 256, 64, 16, 32, 3, 8),   # d=8: 32x8 lattices (conv_stream needs 16-wide ones), 1024 groups
    # LDS-DMA gather GEMM (igemm_dma_kernel): K tail inside the last stage, ragged pixel tile, partial channel tiles, long K ring
    (3, 9, 7, 136, 200, 1, 1),    # 17 K chunks (last step 1/8 full), 189 pixels (second tile partial), N = 128 + 72
    (2, 12, 12, 1024, 40, 1, 1),  # 128 K chunks through the 3-stage ring, 64-wide channel tile with 40 valid
    (1, 6, 10, 40, 8, 1, 1),      # 5 K chunks: shorter than one K step
]

# The kernel each pass of a route-labelled CONV_CASES case lands on (measured on the MI355X with the default thresholds):
# (out_f32 forward, bf16 forward, backward data).  A planner change that moves a case to another kernel fails here first: update
# the label of the case, or add a case that still reaches the named kernel.
_HALO, _PERSIST1, _PERSIST2 = "conv_halo_kernel<1>", "conv_halo_persist_kernel<1>", "conv_halo_persist_kernel<2>"
_BIG, _S14, _S44 = "conv_big_kernel<1, 2, 4>", "conv_stream_kernel<1, 4, false>", "conv_stream_kernel<4, 4, false>"
CONV_ROUTES = {
    (2, 16, 16, 72, 136, 3, 2): (_HALO, _HALO, _HALO),
    (3, 16, 16, 96, 40, 3, 4): (_HALO, _HALO, _HALO),
    (1, 32, 16, 40, 64, 3, 1): (_HALO, _HALO, _HALO),
    (5, 8, 8, 64, 24, 3, 1): (_HALO, _HALO, _HALO),
    (1, 8, 16, 64, 32, 3, 1): (_HALO, "conv_stream_kernel<2, 2, false>", "conv_stream_kernel<4, 2, false>"),
    (2, 32, 32, 256, 64, 3, 1): (_HALO, _HALO, _BIG),
    (1, 128, 128, 64, 64, 3, 1): (_BIG, _BIG, _BIG),
    (2, 32, 32, 64, 64, 3, 8): (_HALO, _HALO, _HALO),
    (1, 32, 32, 48, 24, 3, 4): (_HALO, _HALO, _HALO),
    (1, 64, 32, 88, 16, 3, 2): (_HALO, _S14, _S44),
    (3, 16, 16, 24, 136, 3, 1): (_HALO, _S44, _HALO),
    (1, 64, 64, 8, 16, 3, 1): (_HALO, _S14, _S14),
    (2, 16, 32, 32, 8, 3, 4): (_HALO, _HALO, _HALO),
    (5, 8, 8, 16, 32, 3, 1): (_HALO, _HALO, _HALO),
    (2, 256, 256, 16, 32, 3, 1): (_PERSIST2, "conv_stream_kernel<2, 4, false>", _S14),
    (2, 256, 256, 64, 16, 3, 4): (_BIG, _S14, _S44),
    (5, 256, 128, 24, 8, 3, 2): (_PERSIST1, _S14, "conv_stream_kernel<2, 4, false>"),
    (8, 256, 64, 16, 32, 3, 8): (_PERSIST2, _PERSIST2, _PERSIST1),
    (3, 9, 7, 136, 200, 1, 1): ("igemm_dma_kernel<2, 3>", "igemm_dma_kernel<2, 3>", "igemm_dma_kernel<2, 3>"),
    (2, 12, 12, 1024, 40, 1, 1): ("igemm_dma_kernel<2, 3>", "igemm_dma_kernel<2, 3>", "igemm_dma_kernel<2, 3>"),
    (1, 6, 10, 40, 8, 1, 1): ("igemm_dma_kernel<1, 3>", "igemm_dma_kernel<1, 3>", "igemm_kernel<2, 4>"),
}


# streaming kernel (conv_big.hip conv_stream_kernel): persistent workgroups, weights resident, double-buffered halo DMA.
# (B, H, W, Cin, Cout, dil, forced workgroups or 0): the forced grid drives small shapes through many steps per workgroup.
STREAM_CASES = [
    (8, 256, 256, 32, 32, 1, 0),   # natural plan at 2048 groups: 256-pixel tiles, 4 steps per workgroup, counted wait
    (4, 256, 256, 8, 64, 1, 0),    # fwd: 256-pixel tiles x 64 channels; dgrad 64 -> 8: two resident chunks, 16-channel tile
    (3, 48, 32, 24, 16, 1, 8),     # 18 groups on 8 workgroups: ragged per-XCD split, Cin tail, one workgroup per XCD
    (2, 64, 64, 40, 24, 2, 8),     # dilation 2 (32x32 lattices), two chunks (second partial), Cout 24: partial channel tile
    (5, 32, 64, 16, 40, 1, 16),    # Cout 40 of a 64-wide tile (no counted wait), 40 groups on 16 workgroups
    (1, 128, 128, 32, 32, 4, 8),   # dilation 4 on 128x128: 32x32 lattices, 64 groups: 8 steps per workgroup
]


# (streaming forward, the same forward with the streaming kernel refused, backward data) per STREAM_CASES case
_S = "conv_stream_kernel<{}, {}, {}>".format
STREAM_ROUTES = {
    (8, 256, 256, 32, 32, 1, 0): (_S(2, 4, "false"), "conv_halo_persist_kernel<2>", _S(2, 4, "false")),
    (4, 256, 256, 8, 64, 1, 0): (_S(4, 4, "false"), "conv_halo_persist_kernel<4>", _S(1, 4, "false")),
    (3, 48, 32, 24, 16, 1, 8): (_S(1, 4, "false"), "conv_halo_kernel<1>", _S(2, 4, "false")),
    (2, 64, 64, 40, 24, 2, 8): (_S(2, 4, "false"), "conv_big_kernel<1, 2, 4>", _S(4, 4, "false")),
    (5, 32, 64, 16, 40, 1, 16): (_S(4, 4, "false"), "conv_halo_kernel<1>", _S(1, 4, "false")),
    (1, 128, 128, 32, 32, 4, 8): (_S(2, 4, "false"), "conv_halo_kernel<1>", _S(2, 4, "false")),
}


@pytest.mark.parametrize("B,H,W,Cin,Cout,dil,wgx", STREAM_CASES)
def test_conv_stream(gen, monkeypatch, B, H, W, Cin, Cout, dil, wgx):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    if wgx:
        monkeypatch.setenv("USSEG_STREAM_MIN_STEPS", "1")
        monkeypatch.setenv("USSEG_STREAM_WGX", str(wgx))
    layer = Conv2D(Cin, Cout, 3, dil)
    w = rnd(gen, 3, 3, Cin, Cout, scale=1.0 / math.sqrt(9 * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    ref = O.conv2d_same(x, w, b, dil)
    routes = STREAM_ROUTES[(B, H, W, Cin, Cout, dil, wgx)]
    y = on_route(routes[0], lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3))
    torch.cuda.synchronize()
    assert rel(y[..., :Cout], bf(O.leaky_relu(ref))) < REL_BF16
    assert y[..., Cout:].abs().max().item() == 0 if layer.cout_p > Cout else True
    # the other kernels on the same input must agree to the bf16 bit (same products, fp32 accumulation order aside)
    monkeypatch.setenv("USSEG_STREAM_MIN_STEPS", "1000000")
    y2 = on_route(routes[1], lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3))
    assert rel(y, y2) < 2e-3
    monkeypatch.setenv("USSEG_STREAM_MIN_STEPS", "1" if wgx else "4")
    # backward data through the same kernel (flipped taps, no bias)
    layer.forward(xd)
    dy = rnd(gen, B, H, W, Cout)
    xr = x.clone().requires_grad_(True)
    (O.conv2d_same(xr, w, b, dil) * dy).sum().backward()
    dxd = to_dev_padded(dy)
    dx = on_route(routes[2], lambda: layer.backward(dxd, skip_wgrad=True))
    torch.cuda.synchronize()
    assert rel(dx[..., :Cin], bf(xr.grad)) < 2 * REL_BF16


# (residual forward, the same with the streaming kernel refused).  (1, 32, 48, 16, 16, 2, 8) has 16x24 lattices, which the streaming
# kernel cannot tile: both of its passes are gather GEMMs; (1, 32, 64, 16, 16, 2, 8) is its dilation-2 case that does stream.
STREAM_RES_ROUTES = {
    (2, 128, 128, 30, 64, 1, 0): (_S(4, 4, "true"), "conv_halo_kernel<4>"),
    (2, 64, 64, 32, 30, 1, 8): (_S(2, 4, "true"), "conv_halo_kernel<1>"),
    (1, 32, 48, 16, 16, 2, 8): ("igemm_dma_kernel<1, 3>", "igemm_dma_kernel<1, 3>"),
    (1, 32, 64, 16, 16, 2, 8): (_S(1, 4, "true"), "conv_halo_kernel<1>"),
    (3, 32, 32, 24, 40, 1, 16): (_S(4, 4, "true"), "conv_halo_kernel<1>"),
}


@pytest.mark.parametrize("B,H,W,Cin,Cout,dil,wgx", [(2, 128, 128, 30, 64, 1, 0), (2, 64, 64, 32, 30, 1, 8), (1, 32, 48, 16, 16, 2, 8), (3, 32, 32, 24, 40, 1, 16),
                                                    (1, 32, 64, 16, 16, 2, 8)])
def test_conv_stream_with_residual(gen, monkeypatch, B, H, W, Cin, Cout, dil, wgx):
    """The streaming conv's residual variant (y = act(conv + bias) + residual: concats_2 + shortcut of residual_S, ResNest.py:96-100)
    against the oracle and, to the bf16 bit, against the tiled kernels with the same epilogue."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    monkeypatch.setenv("USSEG_STREAM_MIN_STEPS", "1")
    if wgx:
        monkeypatch.setenv("USSEG_STREAM_WGX", str(wgx))
    layer = Conv2D(Cin, Cout, 3, dil)
    w = rnd(gen, 3, 3, Cin, Cout, scale=1.0 / math.sqrt(9 * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x, r = rnd(gen, B, H, W, Cin), rnd(gen, B, H, W, Cout)
    xd, rd = to_dev_padded(x), to_dev_padded(r)
    ref = O.leaky_relu(O.conv2d_same(x, w, b, dil)) + r
    routes = STREAM_RES_ROUTES[(B, H, W, Cin, Cout, dil, wgx)]
    y = on_route(routes[0], lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3, residual=rd))
    torch.cuda.synchronize()
    assert rel(y[..., :Cout], bf(ref)) < REL_BF16
    assert y[..., Cout:].abs().max().item() == 0 if layer.cout_p > Cout else True
    monkeypatch.setenv("USSEG_STREAM_RES", "0")       # read once per process: compare with the non-streaming kernels through the step planner instead
    monkeypatch.setenv("USSEG_STREAM_MIN_STEPS", "1000000")
    y2 = on_route(routes[1], lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3, residual=rd))
    assert rel(y, y2) < 2e-3


# USSEG_BIG_W8 mode -> (forward, backward data).  conv_big only takes launches of >= 128 workgroups: the small cases run conv_halo
# (or conv_stream) whatever the mode; (2, 32, 32, 256, 64, 1) reaches the eight-wave tile on backward data only and
# (1, 128, 128, 64, 64, 1) on both passes.
_B8, _B4, _H1 = "conv_big_kernel<1, 2, 8>", "conv_big_kernel<1, 2, 4>", "conv_halo_kernel<1>"
EIGHT_WAVE_ROUTES = {
    (2, 32, 32, 256, 64, 1): {"2": (_H1, _B8), "0": (_H1, _B4)},
    (1, 32, 16, 40, 64, 1): {"2": (_H1, _H1), "0": (_H1, _H1)},
    (2, 16, 16, 72, 136, 2): {"2": (_H1, _H1), "0": (_H1, _H1)},
    (3, 16, 16, 96, 40, 4): {"2": (_H1, _H1), "0": (_H1, _H1)},
    (5, 8, 8, 64, 24, 1): {"2": (_H1, _H1), "0": (_H1, _H1)},
    (2, 64, 64, 128, 16, 2): {m: (_S(1, 4, "false"), _S(4, 4, "false")) for m in "20"},
    (1, 128, 128, 64, 64, 1): {"2": (_B8, _B8), "0": (_B4, _B4)},
}


@pytest.mark.parametrize("B,H,W,Cin,Cout,dil", [(2, 32, 32, 256, 64, 1), (1, 32, 16, 40, 64, 1), (2, 16, 16, 72, 136, 2), (3, 16, 16, 96, 40, 4),
                                                (5, 8, 8, 64, 24, 1), (2, 64, 64, 128, 16, 2), (1, 128, 128, 64, 64, 1)])
def test_conv_big_eight_wave_tile(gen, monkeypatch, B, H, W, Cin, Cout, dil):
    """conv_big's 256-pixel tile on eight waves (forced: the planner only picks it for large launches) against the oracle and
    against the four-wave tiles, forward and backward-data (EIGHT_WAVE_ROUTES: which cases reach it)."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    layer = Conv2D(Cin, Cout, 3, dil)
    w = rnd(gen, 3, 3, Cin, Cout, scale=1.0 / math.sqrt(9 * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    ref = O.conv2d_same(x, w, b, dil)
    dy = rnd(gen, B, H, W, Cout)
    xr = x.clone().requires_grad_(True)
    (O.conv2d_same(xr, w, b, dil) * dy).sum().backward()
    outs = []
    for mode in ("2", "0"):
        monkeypatch.setenv("USSEG_BIG_W8", mode)
        want = EIGHT_WAVE_ROUTES[(B, H, W, Cin, Cout, dil)][mode]
        y = on_route(want[0], lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3))
        dyd = to_dev_padded(dy)
        dx = on_route(want[1], lambda: layer.backward(dyd, skip_wgrad=True))
        torch.cuda.synchronize()
        assert rel(y[..., :Cout], bf(O.leaky_relu(ref))) < REL_BF16
        assert rel(dx[..., :Cin], bf(xr.grad)) < 2 * REL_BF16
        outs.append((y.clone(), dx.clone()))
    assert rel(outs[0][0], outs[1][0]) < 2e-3 and rel(outs[0][1], outs[1][1]) < 2e-3


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,dil", CONV_CASES)
def test_conv2d_fwd_dgrad_wgrad(gen, B, H, W, Cin, Cout, k, dil):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    layer = Conv2D(Cin, Cout, k, dil)
    w = rnd(gen, k, k, Cin, Cout, scale=1.0 / math.sqrt(k * k * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    ref = O.conv2d_same(x, w, b, dil)
    mag = O.conv2d_same(x.abs(), w.abs(), b.abs(), dil)         # |x| (*) |w| + |b|: the per-element error scale
    routes = CONV_ROUTES.get((B, H, W, Cin, Cout, k, dil))

    def run(i, fn):     # the kernel a labelled case's pass lands on, asserted before its numbers
        return fn() if routes is None else on_route(routes[i], fn)
    # fp32 output
    y32 = run(0, lambda: layer.forward(xd, out_f32=True))
    torch.cuda.synchronize()
    assert rel(y32[..., :Cout], ref) < REL_F32
    assert_elementwise(y32[..., :Cout], ref, mag, U_F32, 4.0 + math.sqrt(k * k * Cin) / 8, what="fp32 forward")
    # bf16 output: pad channels must be exactly zero
    y16 = run(1, lambda: layer.forward(xd))
    assert rel(y16[..., :Cout], bf(ref)) < REL_BF16
    assert_elementwise(y16[..., :Cout], ref, mag, U_BF16, 4.0, what="bf16 forward")
    assert y16[..., Cout:].abs().max().item() == 0 if layer.cout_p > Cout else True
    # fused LeakyReLU + residual epilogue
    r = rnd(gen, B, H, W, Cout)
    yr = layer.forward(xd, act=ops.ACT_LRELU, alpha=0.3, residual=to_dev_padded(r))
    assert rel(yr[..., :Cout], bf(O.leaky_relu(ref) + r)) < REL_BF16
    assert_elementwise(yr[..., :Cout], O.leaky_relu(ref) + r, mag + r.abs(), U_BF16, 4.0, what="residual forward")
    # backward: dgrad, wgrad, bias grad
    layer.forward(xd)
    dy = rnd(gen, B, H, W, Cout)
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (O.conv2d_same(xr, wr, br, dil) * dy).sum().backward()
    xm, wm = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    (O.conv2d_same(xm, wm, None, dil) * dy.abs()).sum().backward()
    dyd = to_dev_padded(dy)
    dx = run(2, lambda: layer.backward(dyd))
    torch.cuda.synchronize()
    assert rel(dx[..., :Cin], bf(xr.grad)) < REL_BF16
    assert_elementwise(dx[..., :Cin], xr.grad, xm.grad, U_BF16, 4.0, what="backward data")
    if layer.cin_p > Cin:
        assert dx[..., Cin:].abs().max().item() == 0
    assert rel(layer.kernel.grad, wr.grad) < REL_F32
    assert rel(layer.bias.grad, br.grad) < REL_F32
    assert_elementwise(layer.kernel.grad, wr.grad, wm.grad, U_F32, 4.0 + math.sqrt(B * H * W) / 8, what="weight gradient")
    # gradients ACCUMULATE (second backward doubles them)
    layer.backward(to_dev_padded(dy))
    assert rel(layer.kernel.grad, 2 * wr.grad) < REL_F32


def test_conv2d_channel_slices(gen):
    """Producers write into / read from channel slices of concat buffers (ld > C)."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    B, H, W, Cin, Cout = 2, 10, 6, 16, 24
    layer = Conv2D(Cin, Cout, 3, 2)
    w, b = rnd(gen, 3, 3, Cin, Cout, scale=0.1), rnd(gen, Cout)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x = rnd(gen, B, H, W, Cin)
    xbuf = torch.full((B, H, W, 40), 7.0, dtype=torch.bfloat16, device=DEV)
    xbuf[..., 8:24] = x.to(torch.bfloat16).to(DEV)
    ybuf = torch.full((B, H, W, 64), -3.0, dtype=torch.bfloat16, device=DEV)
    layer.forward(xbuf[..., 8:24], out=ybuf[..., 32:56])
    ref = O.conv2d_same(x, w, b, 2)
    assert rel(ybuf[..., 32:56], bf(ref)) < REL_BF16
    assert (ybuf[..., :32] == -3.0).all() and (ybuf[..., 56:] == -3.0).all()
    dy = rnd(gen, B, H, W, Cout)
    dybuf = torch.zeros((B, H, W, 48), dtype=torch.bfloat16, device=DEV)
    dybuf[..., 16:40] = dy.to(torch.bfloat16).to(DEV)
    dxbuf = torch.ones((B, H, W, 32), dtype=torch.bfloat16, device=DEV)
    layer.backward(dybuf[..., 16:40], dx=dxbuf[..., 8:24], accumulate_dx=True)
    xr = x.clone().requires_grad_(True)
    (O.conv2d_same(xr, w, b, 2) * dy).sum().backward()
    assert rel(dxbuf[..., 8:24], bf(xr.grad + 1.0)) < 2 * REL_BF16
    assert (dxbuf[..., :8] == 1.0).all() and (dxbuf[..., 24:] == 1.0).all()


# ------------------------------------------------------------------------------------------------ Conv2DTranspose
TCONV_CASES = [
    (1, 4, 4, 8, 8, 3), (2, 5, 3, 16, 24, 3), (1, 8, 8, 72, 3, 3), (1, 16, 16, 160, 64, 3),
    (1, 4, 4, 8, 8, 4), (2, 3, 5, 24, 16, 4), (1, 8, 8, 160, 3, 4), (1, 1, 1, 16, 8, 4),
    (3, 9, 7, 136, 72, 4), (1, 16, 16, 264, 136, 3),   # parity classes on the LDS-DMA kernel: K tails, ragged pixel tiles, N = 128 + 8
]


# (forward, backward data, weight gradient) of each TCONV_CASES case: the parity-class gather GEMM both ways, the per-tap weight gradient
_G1, _G2, _WD1, _WD2 = "igemm_dma_kernel<1, 3>", "igemm_dma_kernel<2, 3>", "wgrad_dma_kernel<1, 3>", "wgrad_dma_kernel<2, 2>"
TCONV_ROUTES = {
    (1, 4, 4, 8, 8, 3): (_G1, _G1, _WD1), (2, 5, 3, 16, 24, 3): (_G2, _G1, _WD1), (1, 8, 8, 72, 3, 3): (_G1, _G2, _WD1),
    (1, 16, 16, 160, 64, 3): (_G2, _G2, _WD1), (1, 4, 4, 8, 8, 4): (_G1, _G1, _WD1), (2, 3, 5, 24, 16, 4): (_G1, _G2, _WD1),
    (1, 8, 8, 160, 3, 4): (_G1, _G2, _WD1), (1, 1, 1, 16, 8, 4): (_G1, _G1, _WD1), (3, 9, 7, 136, 72, 4): (_G2, _G2, _WD2),
    (1, 16, 16, 264, 136, 3): (_G2, _G2, _WD2),
}
# USSEG_TCONV_HALO -> the weight-gradient kernel: four tap-masked parity-class jobs of wgrad_halo, or the per-tap LDS-DMA kernel
TCONV_WGRAD_HALO_ROUTES = {
    (1, 8, 8, 72, 40, 3): "wgrad_halo_kernel<2, 2, 2, true, 2, true>", (2, 16, 16, 160, 64, 4): "wgrad_halo_kernel<2, 2, 2, true, 2, true>",
    (1, 4, 4, 8, 8, 4): "wgrad_halo_kernel<2, 1, 1, true, 1, true>", (3, 32, 16, 24, 136, 3): "wgrad_halo_kernel<4, 1, 2, true, 1, true>",
}


@pytest.mark.parametrize("B,H,W,Cin,Cout,k", [(1, 8, 8, 72, 40, 3), (2, 16, 16, 160, 64, 4), (1, 4, 4, 8, 8, 4), (3, 32, 16, 24, 136, 3)])
def test_tconv_wgrad_parity_class_halo_form(gen, monkeypatch, B, H, W, Cin, Cout, k):
    """The transposed-conv weight gradient as four tap-masked parity-class jobs of the halo-tile kernel (built, off by default:
    usseg_try_launch_tconv_wgrad_halo) against the oracle and against the per-tap kernel."""
    from ultrasound_modeling_amd.layers import Conv2DTranspose
    w = rnd(gen, k, k, Cout, Cin, scale=1.0 / math.sqrt(k * k * Cin))
    b = rnd(gen, Cout, scale=0.5)
    x = rnd(gen, B, H, W, Cin)
    dy = rnd(gen, B, 2 * H, 2 * W, Cout)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xr, wr, br) * dy).sum().backward()
    grads = []
    for flag in ("1", "0"):
        monkeypatch.setenv("USSEG_TCONV_HALO", flag)
        layer = Conv2DTranspose(Cin, Cout, k)
        layer.kernel.data.copy_(w)
        layer.bias.data.copy_(b)
        finalize(layer)
        layer.forward(to_dev_padded(x))
        dyd = to_dev_padded(dy)
        want = TCONV_WGRAD_HALO_ROUTES[(B, H, W, Cin, Cout, k)] if flag == "1" else "wgrad_dma_kernel<1, 3>"
        on_route(want, lambda: layer.backward(dyd))
        torch.cuda.synchronize()
        assert rel(layer.kernel.grad, wr.grad) < REL_F32
        grads.append(layer.kernel.grad.detach().clone())
    assert rel(grads[0], grads[1]) < 1e-4      # same bf16 products, fp32 sums in a different order


@pytest.mark.parametrize("B,H,W,Cin,Cout,k", TCONV_CASES)
def test_tconv2d_fwd_dgrad_wgrad(gen, B, H, W, Cin, Cout, k):
    from ultrasound_modeling_amd.layers import Conv2DTranspose
    layer = Conv2DTranspose(Cin, Cout, k)
    w = rnd(gen, k, k, Cout, Cin, scale=1.0 / math.sqrt(k * k * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    finalize(layer)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    ref = O.conv2d_transpose_s2_same(x, w, b)
    mag = O.conv2d_transpose_s2_same(x.abs(), w.abs(), b.abs())
    routes = TCONV_ROUTES[(B, H, W, Cin, Cout, k)]
    y32 = on_route(routes[0], lambda: layer.forward(xd, out_f32=True))
    assert rel(y32[..., :Cout], ref) < REL_F32
    assert_elementwise(y32[..., :Cout], ref, mag, U_F32, 4.0 + math.sqrt(k * k * Cin) / 8, what="fp32 forward")
    y16 = on_route(routes[0], lambda: layer.forward(xd))
    assert rel(y16[..., :Cout], bf(ref)) < REL_BF16
    assert_elementwise(y16[..., :Cout], ref, mag, U_BF16, 4.0, what="bf16 forward")
    dy = rnd(gen, B, 2 * H, 2 * W, Cout)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xr, wr, br) * dy).sum().backward()
    xm, wm = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xm, wm, None) * dy.abs()).sum().backward()
    dyd = to_dev_padded(dy)
    dx = on_route(routes[1:], lambda: layer.backward(dyd))
    torch.cuda.synchronize()
    assert rel(dx[..., :Cin], bf(xr.grad)) < REL_BF16
    assert_elementwise(dx[..., :Cin], xr.grad, xm.grad, U_BF16, 4.0, what="backward data")
    assert rel(layer.kernel.grad, wr.grad) < REL_F32
    assert_elementwise(layer.kernel.grad, wr.grad, wm.grad, U_F32, 4.0 + math.sqrt(4 * B * H * W) / 8, what="weight gradient")
    assert rel(layer.bias.grad, br.grad) < REL_F32


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("B,H,W,C,G", [(2, 6, 5, 9, 3), (1, 8, 8, 30, 3), (2, 4, 4, 255, 3), (1, 9, 7, 64, 1),
                                       (1, 3, 3, 512, 1), (2, 5, 5, 84, 3), (1, 4, 4, 8, 4), (1, 2, 2, 5, 1)])
def test_layernorm_grouped_fwd_bwd(gen, B, H, W, C, G):
    from ultrasound_modeling_amd import ops
    x = rnd(gen, B, H, W, C)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    cp = (C + 7) // 8 * 8
    pad = lambda v: torch.cat([v.float(), torch.zeros(cp - C)]).to(DEV)
    xd = to_dev_padded(x)
    Cg = C // G

    def ref_fn(xx, g_, b_):
        parts = [O.layer_norm(xx[..., i * Cg:(i + 1) * Cg], g_[i * Cg:(i + 1) * Cg], b_[i * Cg:(i + 1) * Cg]) for i in range(G)]
        return O.leaky_relu(torch.cat(parts, dim=-1))
    ref = ref_fn(x, gamma, beta)
    y = on_route(kname(False, 0, ng_of(G)), lambda: ops.norm_act_fwd(xd, C, pad(gamma), pad(beta), torch.empty_like(xd), 0, G, 1e-3, ops.ACT_LRELU, 0.3))
    assert rel(y[..., :C], bf(ref)) < REL_BF16
    if cp > C:
        assert y[..., C:].abs().max().item() == 0
    dy = rnd(gen, B, H, W, C)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    (ref_fn(xr, gr, br) * dy).sum().backward()
    dgam, dbet = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    dx = on_route(kname(True, 0, ng_of(G)), lambda: ops.norm_act_bwd(xd, to_dev_padded(dy), C, pad(gamma), pad(beta), torch.empty_like(xd), dgam, dbet,
                                                                     0, G, 1e-3, ops.ACT_LRELU, 0.3))
    assert rel(dx[..., :C], bf(xr.grad)) < 2 * REL_BF16
    assert rel(dgam[:C], gr.grad) < REL_F32
    assert rel(dbet[:C], br.grad) < REL_F32
    M = B * H * W          # every element (test_gpu_norm_routes.py states the bounds)
    r = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), "lrelu", G, dy=dy.reshape(M, C).to(DEV))
    check("LN y", y[..., :C].reshape(M, C), r["y"], r["ymag"], U_BF16, 4.0)
    check_norm_bwd("LN", M, C, r, dx[..., :C].reshape(M, C), dgam, dbet)


@pytest.mark.parametrize("B,H,W,C", [(2, 6, 5, 96), (1, 32, 32, 512), (3, 7, 9, 40), (1, 2, 2, 8)])
def test_layernorm_backward_with_residual(gen, B, H, W, C):
    """usseg_norm_act_bwd_res (the residual branch of a pre-norm transformer block, VisionTransformer.py:137-146 /
    SwinTransformer.py:224-257) == usseg_norm_act_bwd + an accumulating copy, bit for bit; and LN'(dy) + dres against autograd."""
    from ultrasound_modeling_amd import ops
    x, dy, dres = rnd(gen, B, H, W, C), rnd(gen, B, H, W, C), rnd(gen, B, H, W, C)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    xd, dyd, drd = to_dev_padded(x), to_dev_padded(dy), to_dev_padded(dres)
    g, b = gamma.float().to(DEV), beta.float().to(DEV)
    dg1, db1, dg2, db2, dbias, cs = (torch.zeros(C, device=DEV) for _ in range(6))
    sep = ops.norm_act_bwd(xd, dyd, C, g, b, torch.empty_like(xd), dg1, db1, 0, 1, 1e-5)
    ops.copy_channels(drd, sep, accumulate=True)
    ops.colsum(sep, cs, C)
    fused = ops.norm_act_bwd_res(xd, dyd, C, g, b, drd, torch.full_like(xd, float("nan")), dg2, db2, 1e-5, dbias)
    assert torch.equal(fused, sep) and torch.equal(dg1, dg2) and torch.equal(db1, db2)
    # the column sums of the stored result (a Dense bias gradient) without a pass over it
    assert rel(dbias, sep[..., :C].double().sum((0, 1, 2))) < REL_F32 and rel(dbias, cs) < REL_F32
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    (O.layer_norm(xr, gr, br, eps=1e-5) * dy).sum().backward()
    assert rel(fused[..., :C], bf(bf(xr.grad) + dres)) < 2 * REL_BF16      # two roundings, as the separate launches
    assert rel(dg2, gr.grad) < REL_F32 and rel(db2, br.grad) < REL_F32


@pytest.mark.parametrize("C,act", [(32, 1), (16, 1), (64, 3), (24, 2)])
def test_batchnorm_inference_fwd_bwd(gen, C, act):
    from ultrasound_modeling_amd import ops
    B, H, W = 2, 7, 9
    x = rnd(gen, B, H, W, C)
    f = lambda t: t.float().double()
    gamma, beta = f(1 + 0.3 * torch.randn(C, generator=gen)), f(0.2 * torch.randn(C, generator=gen))
    mm, mv = f(0.1 * torch.randn(C, generator=gen)), f(1 + 0.5 * torch.rand(C, generator=gen))
    actf = {1: O.leaky_relu, 2: torch.relu, 3: O.elu}[act]
    alpha = {1: 0.3, 2: 0.0, 3: 1.0}[act]
    d = lambda v: v.float().to(DEV)
    xd = to_dev_padded(x)
    ref = actf(O.batch_norm(x, gamma, beta, mm, mv, training=False))
    y = on_route(kname(False, 1, 1), lambda: ops.norm_act_fwd(xd, C, d(gamma), d(beta), torch.empty_like(xd), 1, 1, 1e-3, act, alpha, d(mm), d(mv)))
    assert rel(y, bf(ref)) < REL_BF16
    dy = rnd(gen, B, H, W, C)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    (actf(O.batch_norm(xr, gr, br, mm, mv, training=False)) * dy).sum().backward()
    dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = on_route(kname(True, 1, 1), lambda: ops.norm_act_bwd(xd, to_dev_padded(dy), C, d(gamma), d(beta), torch.empty_like(xd), dgam, dbet, 1, 1, 1e-3,
                                                              act, alpha, d(mm), d(mv)))
    assert rel(dx, bf(xr.grad)) < REL_BF16
    assert rel(dgam, gr.grad) < REL_F32
    assert rel(dbet, br.grad) < REL_F32
    M, dv = B * H * W, lambda t: t.to(DEV)
    r = norm_ref(x.reshape(M, C).to(DEV), dv(gamma), dv(beta), {1: "lrelu", 2: "relu", 3: "elu"}[act], 1, 1, dv(mm), dv(mv), dy=dy.reshape(M, C).to(DEV))
    check("BN y", y.reshape(M, C), r["y"], r["ymag"], U_BF16, 4.0)
    check_norm_bwd("BN", M, C, r, dx.reshape(M, C), dgam, dbet)


# ------------------------------------------------------------------------------------------------ pooling / copies / cast
def test_avgpool_copy_cast(gen):
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 6, 10, 24
    x = rnd(gen, B, H, W, C)
    xd = to_dev_padded(x)
    y = ops.avgpool2_fwd(xd, ops.new_act(B, H // 2, W // 2, C, DEV))
    assert rel(y, bf(O.avg_pool2(x))) < REL_BF16
    dy, add = rnd(gen, B, H // 2, W // 2, C), rnd(gen, B, H, W, C)
    dx = ops.avgpool2_bwd(to_dev_padded(dy), ops.new_act(B, H, W, C, DEV), to_dev_padded(add))
    ref = dy.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25 + add
    assert rel(dx, bf(ref)) < REL_BF16
    # copy into a channel slice, then accumulate
    dst = torch.zeros(B, H, W, 48, dtype=torch.bfloat16, device=DEV)
    ops.copy_channels(xd, dst[..., 16:40])
    assert torch.equal(dst[..., 16:40], xd) and dst[..., :16].abs().max() == 0
    ops.copy_channels(xd, dst[..., 16:40], accumulate=True)
    assert rel(dst[..., 16:40], bf(2 * x)) < REL_BF16
    # raw row-major reshape re-injection (Decoder.py:140): [B,N,hidden] -> [B,2gh,2gw,hidden/4]
    hid = rnd(gen, 2, 4 * 3, 64)
    hd = hid.to(torch.bfloat16).to(DEV)
    cat = torch.zeros(2, 8, 6, 24, dtype=torch.bfloat16, device=DEV)
    ops.copy_channels(hd.reshape(2, 8, 6, 16), cat[..., 8:])
    assert torch.equal(cat[..., 8:].cpu().double(), hid.reshape(2, 8, 6, 16))
    # input cast fp64 / fp32 -> bf16 with channel padding
    xin = torch.randn(2, 5, 7, 3, generator=gen, dtype=torch.float64)
    for t in (xin, xin.float()):
        c = ops.cast_input(t.to(DEV), 8)
        assert torch.equal(c[..., :3].cpu(), t.to(torch.bfloat16)) and c[..., 3:].abs().max() == 0
    assert torch.equal(ops.to_f32(c, 3).cpu(), c[..., :3].float().cpu())


# ------------------------------------------------------------------------------------------------ split attention
@pytest.mark.parametrize("B,H,W,P,Cg,radix", [(2, 6, 6, 3, 10, 3), (1, 4, 8, 3, 21, 3), (2, 4, 4, 4, 8, 4), (2, 3, 5, 3, 85, 3),
                                              (1, 4, 4, 2, 6, 1)])
def test_split_attention_shared_branches(gen, B, H, W, P, Cg, radix):
    """Arch B form (ResNest.py:171-199 with identical radix branches): out = radix*y*softmax_c(dense2(...)), fwd + bwd."""
    from ultrasound_modeling_amd import ops
    Hd = Cg // 2
    V = P * Cg
    Vp = (V + 7) // 8 * 8
    y = rnd(gen, B, H, W, V)
    f = lambda *s, sc=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * sc).float().double()
    w1, b1 = f(P, Cg, Hd, sc=1 / math.sqrt(Cg)), f(P, Hd, sc=0.1)
    ga, be = 1 + f(P, Hd, sc=0.2), f(P, Hd, sc=0.1)
    w2, b2 = f(P, Hd, Cg, sc=1 / math.sqrt(Hd)), f(P, Cg, sc=0.1)
    dout = rnd(gen, B, H, W, V)

    def ref_fn(yy, w1_, b1_, ga_, be_, w2_, b2_):
        outs = []
        for p in range(P):
            Pd = {"dense1.kernel": w1_[p].reshape(1, 1, Cg, Hd), "dense1.bias": b1_[p], "dense1_bn.gamma": ga_[p], "dense1_bn.beta": be_[p],
                  "dense2.kernel": w2_[p].reshape(1, 1, Hd, Cg), "dense2.bias": b2_[p]}
            yp = yy[..., p * Cg:(p + 1) * Cg]
            outs.append(O.split_attention([yp] * radix, Pd, "", radix))
        return torch.cat(outs, dim=-1)
    leaves = [t.clone().requires_grad_(True) for t in (y, w1, b1, ga, be, w2, b2)]
    ref = ref_fn(*leaves)
    (ref * dout).sum().backward()

    dev = lambda t: t.float().contiguous().to(DEV)
    params = (dev(w1), dev(b1), dev(ga), dev(be), None, None, dev(w2), dev(b2))
    yd = to_dev_padded(y)
    d = ops.splitattn_desc(B, H * W, P, 1, Cg, Hd, Vp, Vp, Vp, Vp, float(radix), 0, 1e-3, ops.ACT_LRELU, 0.3, radix == 1)
    out, g, s, ws = on_route(("sa_reduce_kernel", "sa_mlp_kernel<false>", "sa_apply_kernel<false>"), lambda: ops.splitattn_fwd(d, yd, params, ops.new_act(B, H, W, Vp, DEV)))
    assert rel(out[..., :V], bf(ref)) < REL_BF16
    grads = tuple(torch.zeros_like(t) for t in (params[0], params[1], params[2], params[3], params[6], params[7]))
    dy = on_route(("sa_reduce_kernel", "sa_mlp_kernel<true>", "sa_apply_kernel<true>"), lambda: ops.splitattn_bwd(d, yd, to_dev_padded(dout), params, grads, g, s, ws, torch.empty_like(yd)))
    assert rel(dy[..., :V], bf(leaves[0].grad)) < 2 * REL_BF16
    for got, want in zip(grads, (leaves[1].grad, leaves[2].grad, leaves[3].grad, leaves[4].grad, leaves[5].grad, leaves[6].grad)):
        assert rel(got, want) < 2e-3, (got.shape,)
    torch.cuda.synchronize()
    prm = [t.to(DEV) for t in (w1, b1, ga, be, torch.zeros(P, Hd, dtype=torch.float64), torch.ones(P, Hd, dtype=torch.float64), w2.unsqueeze(1), b2.unsqueeze(1))]
    r = sa_reference(y.reshape(B, H * W, V).to(DEV), dout.reshape(B, H * W, V).to(DEV), prm, P, 1, Cg, Hd, float(radix), 0, "lrelu", radix == 1)
    check("sa out", out[..., :V].reshape(B, H * W, V), r["out"], r["outm"], U_BF16, 4.0)
    check("sa dy", dy[..., :V].reshape(B, H * W, V), r["dy"], r["dym"], U_BF16, 4.0)
    for got, want, mag in zip(grads, (r["grads"][0], r["grads"][1], r["grads"][2], r["grads"][3], r["grads"][4][:, 0], r["grads"][5][:, 0]),
                              (r["gmags"][0], r["gmags"][1], r["gmags"][2], r["gmags"][3], r["gmags"][4][:, 0], r["gmags"][5][:, 0])):
        check("sa gradient", got, want, mag, U_F32, c_f32(B * H * W))


@pytest.mark.parametrize("B,H,W,P,Cg,R", [(2, 6, 6, 4, 8, 3), (1, 4, 8, 2, 64, 3), (2, 4, 4, 4, 16, 3), (2, 3, 5, 3, 10, 3), (2, 8, 8, 2, 32, 2),
                                         (1, 4, 4, 2, 6, 1)])
def test_split_attention_distinct_branches(gen, B, H, W, P, Cg, R):
    """Arch A form (TBI_ResNest.py:175-207): R DIFFERENT branch tensors per path, dense1 + BatchNormalization (moving statistics) + ELU,
    one dense2 PER radix branch, softmax over channels (sigmoid if R == 1), out = sum_r y_r * z_r written into a channel slice of a
    wider concat buffer - forward, dy and every MLP gradient."""
    from ultrasound_modeling_amd import ops
    Hd = Cg // 2
    V, Co = P * R * Cg, P * Cg
    Vp, Cop = (V + 7) // 8 * 8, (Co + 7) // 8 * 8
    y = rnd(gen, B, H, W, V)
    f = lambda *s, sc=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * sc).float().double()
    w1, b1 = f(P, Cg, Hd, sc=1 / math.sqrt(Cg)), f(P, Hd, sc=0.1)
    ga, be = 1 + f(P, Hd, sc=0.2), f(P, Hd, sc=0.1)
    mm, mv = f(P, Hd, sc=0.2), 0.5 + torch.rand(P, Hd, generator=gen, dtype=torch.float64).float().double()
    w2, b2 = f(P, R, Hd, Cg, sc=1 / math.sqrt(Hd)), f(P, R, Cg, sc=0.1)
    dout = rnd(gen, B, H, W, Co)

    def ref_fn(yy, w1_, b1_, ga_, be_, w2_, b2_):
        outs = []
        for p in range(P):
            Pd = {"a1.kernel": w1_[p].reshape(1, 1, Cg, Hd), "a1.bias": b1_[p], "a_bn.gamma": ga_[p], "a_bn.beta": be_[p],
                  "a_bn.moving_mean": mm[p], "a_bn.moving_variance": mv[p]}
            for r in range(R):
                Pd[f"a2_r{r}.kernel"], Pd[f"a2_r{r}.bias"] = w2_[p, r].reshape(1, 1, Hd, Cg), b2_[p, r]
            ins = [yy[..., (p * R + r) * Cg:(p * R + r + 1) * Cg] for r in range(R)]
            outs.append(O.archA_split_attention(ins, Pd, "a"))
        return torch.cat(outs, dim=-1)
    leaves = [t.clone().requires_grad_(True) for t in (y, w1, b1, ga, be, w2, b2)]
    ref = ref_fn(*leaves)
    (ref * dout).sum().backward()

    dev = lambda t: t.float().contiguous().to(DEV)
    params = (dev(w1), dev(b1), dev(ga), dev(be), dev(mm), dev(mv), dev(w2), dev(b2))
    yd = to_dev_padded(y)
    cat = ops.new_act(B, H, W, Cop + 16, DEV, zero=True)          # the stage's concats_1 buffer: this slab owns channels [8, 8 + Co)
    out = cat[..., 8:8 + Cop]
    d = ops.splitattn_desc(B, H * W, P, R, Cg, Hd, Vp, Cop + 16, Vp, Cop, 1.0, 1, 1e-3, ops.ACT_ELU, 1.0, R == 1)
    _, g, s, ws = on_route(("sa_reduce_kernel", "sa_mlp_kernel<false>", "sa_apply_kernel<false>"), lambda: ops.splitattn_fwd(d, yd, params, out))
    assert rel(out[..., :Co], bf(ref)) < REL_BF16
    assert cat[..., :8].abs().max().item() == 0 and cat[..., 8 + Cop:].abs().max().item() == 0
    grads = tuple(torch.zeros_like(t) for t in (params[0], params[1], params[2], params[3], params[6], params[7]))
    dcat = ops.new_act(B, H, W, Cop + 16, DEV, zero=True)
    dcat[..., 8:8 + Co] = dout.to(torch.bfloat16).to(DEV)
    dy = on_route(("sa_reduce_kernel", "sa_mlp_kernel<true>", "sa_apply_kernel<true>"), lambda: ops.splitattn_bwd(d, yd, dcat[..., 8:8 + Cop], params, grads, g, s, ws, torch.empty_like(yd)))
    torch.cuda.synchronize()
    assert rel(dy[..., :V], bf(leaves[0].grad)) < 2 * REL_BF16
    assert Vp == V or dy[..., V:].abs().max().item() == 0
    for got, want in zip(grads, (leaves[1].grad, leaves[2].grad, leaves[3].grad, leaves[4].grad, leaves[5].grad, leaves[6].grad)):
        assert rel(got, want) < 2e-3, (got.shape,)
    r = sa_reference(y.reshape(B, H * W, V).to(DEV), dout.reshape(B, H * W, Co).to(DEV), [t.to(DEV) for t in (w1, b1, ga, be, mm, mv, w2, b2)],
                     P, R, Cg, Hd, 1.0, 1, "elu", R == 1)
    check("sa out", out[..., :Co].reshape(B, H * W, Co), r["out"], r["outm"], U_BF16, 4.0)
    check("sa dy", dy[..., :V].reshape(B, H * W, V), r["dy"], r["dym"], U_BF16, 4.0)
    for got, want, mag in zip(grads, r["grads"], r["gmags"]):
        check("sa gradient", got, want, mag, U_F32, c_f32(B * H * W))


@pytest.mark.parametrize("B,H,W,P,Cg,radix", [(2, 8, 8, 3, 10, 3), (3, 16, 8, 3, 21, 3), (2, 4, 4, 3, 85, 3), (2, 32, 32, 3, 42, 3)])
def test_split_attention_folded_into_its_norms(gen, B, H, W, P, Cg, radix):
    """The residual_S chain LayerNorm+LeakyReLU -> split attention (ResNest.py:143-147,171-199) as the model runs it: the norm
    launch also emits the pooled partial rows (no pooling pass), and the norm BACKWARD forms the re-weighting's backward
    radix*s*dout + dg in registers (no apply pass, no dy tensor) - against the oracle chain, forward and every gradient."""
    from ultrasound_modeling_amd import ops
    Hd, V = Cg // 2, P * Cg
    Vp = (V + 7) // 8 * 8
    v_raw = bf(rnd(gen, B, H, W, V) * 1.5 + 0.2)
    f = lambda *s, sc=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * sc).float().double()
    g2, be2 = 1 + f(V, sc=0.2), f(V, sc=0.1)
    w1, b1 = f(P, Cg, Hd, sc=1 / math.sqrt(Cg)), f(P, Hd, sc=0.1)
    ga, be = 1 + f(P, Hd, sc=0.2), f(P, Hd, sc=0.1)
    w2, b2 = f(P, Hd, Cg, sc=1 / math.sqrt(Hd)), f(P, Cg, sc=0.1)
    dout = rnd(gen, B, H, W, V)
    leaves = [t.clone().requires_grad_(True) for t in (v_raw, g2, be2, w1, b1, ga, be, w2, b2)]
    vr, g2_, be2_, w1_, b1_, ga_, be_, w2_, b2_ = leaves
    outs, ys = [], []
    for p in range(P):
        sl = slice(p * Cg, (p + 1) * Cg)
        yp = O.leaky_relu(O.layer_norm(vr[..., sl], g2_[sl], be2_[sl]))
        ys.append(yp)
        Pd = {"dense1.kernel": w1_[p].reshape(1, 1, Cg, Hd), "dense1.bias": b1_[p], "dense1_bn.gamma": ga_[p], "dense1_bn.beta": be_[p],
              "dense2.kernel": w2_[p].reshape(1, 1, Hd, Cg), "dense2.bias": b2_[p]}
        outs.append(O.split_attention([bf(yp.detach()) + (yp - yp.detach())] * radix, Pd, "", radix))   # the pool sees the STORED (bf16) y
    ref = torch.cat(outs, -1)
    (ref * dout).sum().backward()

    dev = lambda t: t.float().contiguous().to(DEV)
    pad = lambda t: torch.cat([t.float(), torch.zeros(Vp - V)]).to(DEV)
    params = (dev(w1), dev(b1), dev(ga), dev(be), None, None, dev(w2), dev(b2))
    xd = to_dev_padded(v_raw)
    gam, bet = pad(g2), pad(be2)
    y, gap = on_route(kname(False, 0, 3, fuse=True), lambda: ops.norm_act_fwd_gap(xd, V, gam, bet, torch.empty_like(xd), 0, P, 1e-3, ops.ACT_LRELU, 0.3))
    y_plain = ops.norm_act_fwd(xd, V, gam, bet, torch.empty_like(xd), 0, P, 1e-3, ops.ACT_LRELU, 0.3)
    assert torch.equal(y, y_plain)                                   # same values as the plain launch, bit for bit
    pooled = gap[0].sum(dim=1)[:, :V] / (H * W)
    assert rel(pooled, y[..., :V].float().mean(dim=(1, 2))) < 1e-5
    d = ops.splitattn_desc(B, H * W, P, 1, Cg, Hd, Vp, Vp, Vp, Vp, float(radix), 0, 1e-3, ops.ACT_LRELU, 0.3, radix == 1)
    out, g, s, ws = on_route(("sa_mlp_kernel<false>", "sa_apply_kernel<false>"), lambda: ops.splitattn_fwd(d, y, params, ops.new_act(B, H, W, Vp, DEV), gap=gap))
    assert rel(out[..., :V], bf(ref)) < REL_BF16
    out2, *_ = ops.splitattn_fwd(d, y, params, ops.new_act(B, H, W, Vp, DEV))       # the pooling-pass form agrees
    assert rel(out, out2) < 1e-3
    grads = tuple(torch.zeros_like(t) for t in (params[0], params[1], params[2], params[3], params[6], params[7]))
    doutd = to_dev_padded(dout)
    sa_s, sa_dg = on_route(("sa_reduce_kernel", "sa_mlp_kernel<true>"), lambda: ops.splitattn_bwd(d, y, doutd, params, grads, g, s, ws, None))
    dgam, dbet, dbias = torch.zeros(Vp, device=DEV), torch.zeros(Vp, device=DEV), torch.zeros(Vp, device=DEV)
    dv = on_route(kname(True, 0, 3, fuse=True), lambda: ops.norm_act_bwd_sa(xd, doutd, V, gam, bet, torch.empty_like(xd), dgam, dbet, 0, P, 1e-3,
                                                                           ops.ACT_LRELU, 0.3, sa_s, sa_dg, float(radix), dbias=dbias))
    torch.cuda.synchronize()
    assert rel(dv[..., :V], bf(vr.grad)) < 2 * REL_BF16
    assert Vp == V or dv[..., V:].abs().max().item() == 0
    assert rel(dgam[:V], g2_.grad) < 2e-3 and rel(dbet[:V], be2_.grad) < 2e-3
    assert rel(dbias[:V], vr.grad.sum(dim=(0, 1, 2))) < 2e-3
    for got, want in zip(grads, (w1_.grad, b1_.grad, ga_.grad, be_.grad, w2_.grad, b2_.grad)):
        assert rel(got, want) < 2e-3, (got.shape,)
    # every element: y against the LayerNorm, the split attention on the kernel's own y, and dv from the kernel's own (s, dg)
    M, HW = B * H * W, H * W
    x64, do64 = v_raw.reshape(M, V).to(DEV), dout.reshape(M, V).to(DEV)
    ry = norm_ref(x64, g2.to(DEV), be2.to(DEV), "lrelu", P)
    check("folded y", y[..., :V].reshape(M, V), ry["y"], ry["ymag"], U_BF16, 4.0)
    prm = [t.to(DEV) for t in (w1, b1, ga, be, torch.zeros(P, Hd, dtype=torch.float64), torch.ones(P, Hd, dtype=torch.float64), w2.unsqueeze(1), b2.unsqueeze(1))]
    r = sa_reference(y[..., :V].double().reshape(B, HW, V), do64.view(B, HW, V), prm, P, 1, Cg, Hd, float(radix), 0, "lrelu", radix == 1)
    check("folded sa out", out[..., :V].reshape(B, HW, V), r["out"], r["outm"], U_BF16, 4.0)
    se, ge = (t.double().repeat_interleave(HW, 0) for t in (sa_s, sa_dg))
    rd = norm_ref(x64, g2.to(DEV), be2.to(DEV), "lrelu", P, dy=radix * se * do64 + ge)
    rm = norm_ref(x64, g2.to(DEV), be2.to(DEV), "lrelu", P, dy=radix * se * do64.abs() + ge.abs())
    rd.update({k: rm[k] for k in ("dxmag", "dxext", "dgmag", "dbmag", "dgext", "dbext")}, kink=rd["kink"] | rm["kink"])
    check_norm_bwd("folded", M, V, rd, dv[..., :V].reshape(M, V), dgam, dbet, dbias)


@pytest.mark.parametrize("B,H,W,C,act", [(2, 16, 16, 32, "lrelu"), (3, 8, 12, 24, "elu"), (1, 64, 32, 32, "lrelu")])
def test_bn_act_pool_one_pass(gen, B, H, W, C, act):
    """Inference BatchNorm + activation + AveragePooling2D(2,2) in one launch (the stems, ResNest.py:45-47 / TBI_ResNest.py:90-92):
    bit-identical to the two-launch form, and within tolerance of the oracle, forward and backward."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import AveragePooling2D, BatchNormalization
    A, alpha, fa = (ops.ACT_LRELU, 0.3, O.leaky_relu) if act == "lrelu" else (ops.ACT_ELU, 1.0, O.elu)
    bn = BatchNormalization(C)
    finalize(bn)
    f = lambda *s, sc=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * sc).float().double()
    gam, bet, mean, var = 1 + f(C, sc=0.2), f(C, sc=0.1), f(C, sc=0.3), 0.5 + torch.rand(C, generator=gen, dtype=torch.float64).float().double()
    bn.gamma.data.copy_(gam); bn.beta.data.copy_(bet); bn.moving_mean_p[:C] = mean.float().to(DEV); bn.moving_variance_p[:C] = var.float().to(DEV)
    x = rnd(gen, B, H, W, C) * 1.3
    x = bf(x)
    dy = rnd(gen, B, H // 2, W // 2, C)
    xl, gl, bl = (t.clone().requires_grad_(True) for t in (x, gam, bet))
    ref = O.avg_pool2(fa(O.batch_norm(xl, gl, bl, mean, var)))
    gx, gg, gb = torch.autograd.grad(ref, [xl, gl, bl], dy)
    xd, dyd = to_dev_padded(x), to_dev_padded(dy)
    pooled = on_route("bn_act_pool_kernel<false>", lambda: bn.forward_pool(xd, A, alpha))
    two = AveragePooling2D()
    want = two.forward(bn.forward(xd, A, alpha))
    assert torch.equal(pooled, want)
    # the four activated values are rounded to bf16 before they are averaged (what the two-launch form stored), then the mean is
    # rounded: ~2.5e-3 against the single-rounding fp64 result - the bit-identity above is the kernel check
    assert rel(pooled[..., :C], bf(ref)) < 4e-3
    bn.gamma.grad.zero_(); bn.beta.grad.zero_()
    db = torch.zeros((C + 7) // 8 * 8, device=DEV)
    dx = on_route(kname(True, 1, 1, pool=True), lambda: bn.backward_pool(dyd, dbias=db))
    torch.cuda.synchronize()
    M, dv = B * H * W, lambda t: t.to(DEV)
    dyu = (dy.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25).reshape(M, C).to(DEV)
    r = norm_ref(x.reshape(M, C).to(DEV), dv(gam), dv(bet), act, 1, 1, dv(mean), dv(var), dy=dyu)
    pool = lambda t: t.reshape(B, H // 2, 2, W // 2, 2, C).mean((2, 4))
    check("pool y", pooled[..., :C], pool(r["y"]), pool(r["ymag"]), U_BF16, 4.0)
    check_norm_bwd("pool", M, C, r, dx[..., :C].reshape(M, C), bn.gamma.grad, bn.beta.grad, db)
    g1, b1 = bn.gamma.grad.clone(), bn.beta.grad.clone()
    bn.gamma.grad.zero_(); bn.beta.grad.zero_()
    db2 = torch.zeros_like(db)
    bn.forward(xd, A, alpha)
    dx2 = bn.backward(two.backward(dyd), dbias=db2)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    assert rel(g1, bn.gamma.grad) < 1e-5 and rel(b1, bn.beta.grad) < 1e-5 and rel(db, db2) < 1e-5
    assert rel(dx[..., :C], bf(gx)) < REL_BF16 and rel(g1, gg) < 2e-3 and rel(b1, gb) < 2e-3 and rel(db[:C], gx.sum(dim=(0, 1, 2))) < 2e-3


def test_act_bwd_with_column_sums(gen):
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 9, 7, 16
    x, dy = rnd(gen, B, H, W, C), rnd(gen, B, H, W, C)
    xd, dyd = to_dev_padded(x), to_dev_padded(dy)
    db = torch.zeros(C, device=DEV)
    dx = ops.act_bwd_colsum(xd, dyd, torch.empty_like(dyd), ops.ACT_LRELU, 0.3, db, C)
    dx2 = ops.act_bwd(xd, dyd, torch.empty_like(dyd), ops.ACT_LRELU, 0.3)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    assert rel(db, dx2.float().sum(dim=(0, 1, 2))) < 1e-5


# ------------------------------------------------------------------------------------------------ loss / optimiser
@pytest.mark.parametrize("C", [3, 2, 4])       # 3: the unrolled kernel of the reference's class count; others: the run-time class loop
def test_softmax_cce_loss_fwd_bwd(gen, C):
    from ultrasound_modeling_amd import ops
    B, H, W = 2, 9, 11
    logits = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64).float().double() * 3
    logits[0, 0, 0] = torch.tensor([40.0, -40.0, 0.0, 0.0][:C])   # forces the 1e-7 clip branch
    if C == 3:
        x_, y = O.synthetic_batch(B, 16, 16, 1, seed=3)
        y = y[:, :H, :W].float().double()
    else:
        y = torch.softmax(2 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float64), -1).float().double()
    lr = logits.clone().requires_grad_(True)
    probs_ref = O.softmax_lastaxis(lr)
    loss_ref = O.compute_loss(y, probs_ref, global_batch_size=4)
    loss_ref.backward()
    lg = torch.zeros(B, H, W, 4)
    lg[..., :C] = logits.float()
    lg = lg.to(DEV)
    probs = torch.empty(B, H, W, C, device=DEV)
    loss = torch.zeros(ops.ACC_FLOATS, device=DEV)            # reproducible accumulator: [0] is the scalar
    dl = ops.new_act(B, H, W, 8, DEV)
    ops.softmax_loss(lg, y.float().to(DEV), probs, loss, dl, HW=H * W, C_classes=C, inv_global_batch=0.25)
    assert rel(probs, probs_ref.detach()) < 1e-5
    assert abs(loss[0].item() - loss_ref.item()) / abs(loss_ref.item()) < 1e-5
    assert loss[1].item() == 0                                # the ticket counter is back at zero
    assert rel(dl[..., :C], bf(lr.grad)) < REL_BF16
    assert dl[..., C:].abs().max().item() == 0


def test_clip_adam_matches_oracle(gen):
    from ultrasound_modeling_amd import ops
    n = 10007
    p = torch.randn(n, generator=gen, dtype=torch.float64).float()
    pad = (n + 7) // 8 * 8
    P, G = torch.zeros(pad), torch.zeros(pad)
    P[:n] = p
    pd, gd, m, v = P.to(DEV), G.to(DEV), torch.zeros(pad, device=DEV), torch.zeros(pad, device=DEV)
    step, lr_t, ss = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.zeros(ops.ACC_FLOATS, device=DEV)
    po = [p.double().clone()]
    mo, vo = [torch.zeros(n, dtype=torch.float64)], [torch.zeros(n, dtype=torch.float64)]
    for it in range(1, 4):
        g = torch.randn(n, generator=gen, dtype=torch.float64).float() * (5.0 if it != 2 else 1e-3)   # clipped / not clipped
        gd[:n] = g.to(DEV)
        ops.fill_f32(ss, 0.0)
        ops.sumsq(gd, ss)
        assert abs(ss[0].item() - (g.double() ** 2).sum().item()) / (g.double() ** 2).sum().item() < 1e-5
        ops.adam_advance(step, lr_t, 1e-3, 0.9, 0.999)
        ops.adam_clip_step(pd, gd, m, v, ss, 1.0, lr_t, 0.9, 0.999, 1e-7)
        clipped, _ = O.clip_by_global_norm([g.double()])
        O.adam_step(po, clipped, mo, vo, it, 1e-3)
        assert rel(pd[:n], po[0]) < 1e-6
    assert step.item() == 3


def test_batchnorm_training_mode(gen):
    """Keras training=True semantics: batch mean / biased variance, moving statistics with momentum 0.99,
    and the full batch-statistics backward."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import BatchNormalization
    B, H, W, C = 3, 10, 6, 24
    x = rnd(gen, B, H, W, C) * 1.5 + 0.3
    x = bf(x)
    bn = BatchNormalization(C)
    ga, be = (1 + 0.3 * torch.randn(C, generator=gen)).double(), (0.2 * torch.randn(C, generator=gen)).double()
    bn.gamma.data.copy_(ga)
    bn.beta.data.copy_(be)
    finalize(bn)
    bn.training_mode = True
    xd = to_dev_padded(x)
    xr, gr, br = x.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    y_ref, (mm, mv) = O.batch_norm(xr, gr, br, torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), training=True)
    y_ref = O.leaky_relu(y_ref)
    y = on_route(("colsum_kernel<2>", "bn_batch_finalize_kernel", kname(False, 1, 1)), lambda: bn.forward(xd, ops.ACT_LRELU, 0.3))
    assert rel(y, bf(y_ref)) < 2e-3
    assert rel(bn.moving_mean, mm) < 1e-4 and rel(bn.moving_variance, mv) < 1e-4
    dy = rnd(gen, B, H, W, C)
    (y_ref * dy).sum().backward()
    dx = on_route((kname(True, 1, 1), "bn_train_bwd_fix_kernel"), lambda: bn.backward(to_dev_padded(dy)))
    assert rel(dx, bf(xr.grad)) < 5e-3
    assert rel(bn.gamma.grad, gr.grad) < 2e-3 and rel(bn.beta.grad, br.grad) < 2e-3
    M = B * H * W
    x64 = x.reshape(M, C).to(DEV)
    r = norm_ref(x64, ga.to(DEV), be.to(DEV), "lrelu", mode="batch", dy=dy.reshape(M, C).to(DEV))
    var = ((x64 - x64.mean(0)) ** 2).mean(0)
    check("batch mean", bn._bmean[:C], x64.mean(0), x64.abs().mean(0), U_F32, c_f32(M))
    check("batch variance", bn._bvar[:C], var, var, U_F32, c_f32(M))
    check("moving mean", bn.moving_mean, r["stats"][0], 0.01 * x64.abs().mean(0), U_F32, c_f32(M))
    check("moving variance", bn.moving_variance, r["stats"][1], 0.99 + 0.01 * var, U_F32, c_f32(M))
    check("batch y", y.reshape(M, C), r["y"], r["ymag"], U_BF16, 4.0)
    check_norm_bwd("batch", M, C, r, dx.reshape(M, C), bn.gamma.grad, bn.beta.grad)


# ------------------------------------------------------------------------------------------------ decoder-stage entry points
@pytest.mark.parametrize("B,H,W,Cin,q", [(2, 16, 16, 40, 8), (1, 32, 32, 128, 16), (2, 16, 16, 72, 24)])
def test_decoder_stage_multi_job_and_fused_dgrad(gen, B, H, W, Cin, q):
    """The DecoderBlock stage (Decoder.py:67-75): 1x1 + three dilated 3x3 convs on one input.
    usseg_conv2d_fwd_multi == the convs one by one; usseg_conv2d_dgrad_branches == the sum of their backward-data passes;
    usseg_conv2d_wgrad_multi == the weight gradients one by one; all against the fp64 oracle."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    dil, ks = (1, 2, 4, 8), (1, 3, 3, 3)
    convs, ws, bs = [], [], []
    holder = torch.nn.ModuleList()
    for j in range(4):
        c = Conv2D(Cin, q, ks[j], dil[j])
        w = rnd(gen, ks[j], ks[j], Cin, q, scale=1.0 / math.sqrt(ks[j] * ks[j] * Cin))
        b = rnd(gen, q, scale=0.5)
        c.kernel.data.copy_(w); c.bias.data.copy_(b)
        convs.append(c); ws.append(w); bs.append(b); holder.append(c)
    finalize(holder)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    cin_p = xd.shape[-1]
    refs = [O.conv2d_same(x, ws[j], bs[j], dil[j]) for j in range(4)]
    out = torch.zeros(B, H, W, 4 * q, dtype=torch.bfloat16, device=DEV)
    for c in convs:
        c._x = xd
    convs[0].forward(xd, out=out[..., :q])
    ops.conv2d_fwd_multi([(xd, c.wp_f, c.bias.data, c.k, c.dil, out[..., j * q:(j + 1) * q], ops.ACT_NONE, 0.0)
                          for j, c in enumerate(convs) if j > 0])
    torch.cuda.synchronize()
    for j in range(4):
        assert rel(out[..., j * q:(j + 1) * q], bf(refs[j])) < REL_BF16, j
    # backward
    dy = rnd(gen, B, H, W, 4 * q)
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    sum((O.conv2d_same(xr, wr[j], bs[j], dil[j]) * dy[..., j * q:(j + 1) * q]).sum() for j in range(4)).backward()
    dyd = to_dev_padded(dy)
    wcat = torch.zeros((ops.roundup(cin_p, 16), 28 * q), dtype=torch.bfloat16, device=DEV)
    jobs, base = [], 0
    for c in convs:
        T = c.k * c.k
        sT, sI, sO = c._strides_tio()
        jobs.append(ops.pack_job(c.kernel.data, sT, sI, sO, T, c.cin, c.cout, wcat, 28 * q, q, 0, base))
        base += T * q
    ops.pack_weights_batched(ops.make_pack_table(jobs, DEV), len(jobs))
    dx = torch.full((B, H, W, cin_p), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.conv2d_dgrad_branches(dyd, wcat, [c.k for c in convs], [c.dil for c in convs], [j * q for j in range(4)], q, dx)
    torch.cuda.synchronize()
    assert rel(dx[..., :Cin], bf(xr.grad)) < 2 * REL_BF16
    if cin_p > Cin:
        assert dx[..., Cin:].abs().max().item() == 0
    ops.conv2d_wgrad_multi([convs[j].wgrad_job(dyd[..., j * q:(j + 1) * q]) for j in (1, 2, 3)])
    torch.cuda.synchronize()
    for j in (1, 2, 3):
        assert rel(convs[j].kernel.grad, wr[j].grad) < REL_F32, j


@pytest.mark.parametrize("B,H,W,chans", [(2, 64, 64, ((32, 32), (16, 32), (1, 16))), (1, 32, 48, ((24, 32), (32, 24), (8, 8))),
                                         (2, 32, 32, ((64, 128), (24, 64))), (1, 16, 16, ((256, 64), (128, 128)))])
def test_weight_gradients_of_different_channel_counts_in_one_launch(gen, B, H, W, chans):
    """usseg_conv2d_wgrad_multi with jobs of DIFFERENT channel counts that take the same tile shape and tile count (the stem's three convs,
    ResNest.py:39-44; a stage's conv2 and concats_2): each gradient against the fp64 oracle and against its own launch (other split-K counts:
    fp32-level agreement, not bit equality)."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    holder = torch.nn.ModuleList([Conv2D(ci, co, 3) for ci, co in chans])
    finalize(holder)
    jobs, refs = [], []
    for c, (ci, co) in zip(holder, chans):
        x, dy = rnd(gen, B, H, W, ci), rnd(gen, B, H, W, co)
        wr = torch.zeros(3, 3, ci, co, dtype=torch.float64, requires_grad=True)
        (O.conv2d_same(x, wr, torch.zeros(co, dtype=torch.float64), 1) * dy).sum().backward()
        refs.append(wr.grad)
        c._x = to_dev_padded(x)
        jobs.append(c.wgrad_job(to_dev_padded(dy)))
    ops.conv2d_wgrad_multi(jobs)
    torch.cuda.synchronize()
    merged = [c.kernel.grad.clone() for c in holder]
    for c, r in zip(holder, refs):
        assert rel(c.kernel.grad, r) < REL_F32
        c.kernel.grad.zero_()
    for c, job in zip(holder, jobs):
        ops.conv2d_wgrad_multi([job])
    torch.cuda.synchronize()
    for c, m in zip(holder, merged):
        assert rel(c.kernel.grad, m) < 1e-5


def test_deferred_finishing_matches_immediate(gen):
    """usseg_defer_begin/_end: the queued, batched finishing reductions give the same gradients as the immediate ones."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D, LayerNormalization
    B, H, W, Cin, Cout = 2, 16, 16, 24, 40
    holder = torch.nn.ModuleList([Conv2D(Cin, Cout, 3), LayerNormalization(Cout), Conv2D(Cout, 21, 1)])
    conv, ln, conv2 = holder
    finalize(holder)
    x = to_dev_padded(rnd(gen, B, H, W, Cin))
    dy = to_dev_padded(rnd(gen, B, H, W, 21))

    def run(deferred):
        for p in holder.parameters():
            p.grad.zero_()
        r = conv.forward(x)
        a = ln.forward(r, ops.ACT_LRELU, 0.3)
        conv2.forward(a)
        ctx = ops.overlap_region() if deferred else __import__("contextlib").nullcontext()

        def backward():
            with ctx:
                d = conv2.backward(dy)
                d = ln.backward(d, dbias=conv.bias.grad)
                conv.backward(d, need_dx=False, skip_bias=True)
        # deferred: the queued finishing reductions run as one batched launch; immediate: one finishing launch per weight gradient
        _, got = kernels(backward)
        got = [short(n) for n in got]
        finish = "wgrad_finish_batched_kernel" if deferred else "wgrad_finish_kernel"
        other = "wgrad_finish_kernel" if deferred else "wgrad_finish_batched_kernel"
        assert finish in got and other not in got, got
        torch.cuda.synchronize()
        return [p.grad.clone() for p in holder.parameters()]

    g0, g1 = run(False), run(True)
    for a, b in zip(g0, g1):
        assert rel(b, a) < 1e-5


def test_head_quad_form_matches_transposed_conv(gen):
    """The 3-class head Conv2DTranspose(3x3, s2) (Decoder.py:120) run as a 2x2-tap conv with 16 parity channels: forward
    logits, softmax/loss in the quad layout and all three gradients against the plain transposed-conv path."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    import ultrasound_modeling_amd.Decoder as D
    torch.manual_seed(5)
    x = torch.randn(2, 64, 64, 1).clamp_(-1, 1)
    y = torch.softmax(torch.randn(2, 64, 64, 3), -1)
    res = []
    for quad in ("1", "0"):
        import os
        os.environ["USSEG_QUAD_HEAD"] = quad
        torch.manual_seed(11)
        net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1)
        assert net.decoder.quad_head == (quad == "1")
        loss, probs = net.train_step(x, y)
        torch.cuda.synchronize()
        res.append((loss.item(), probs.clone(), net.decoder.head.kernel.data.clone(), net.decoder.head.bias.data.clone(),
                    net.flat.flat.clone()))
    os.environ.pop("USSEG_QUAD_HEAD")
    (l1, p1, k1, b1, f1), (l0, p0, k0, b0, f0) = res
    assert abs(l1 - l0) < 2e-3 * abs(l0) and rel(p1, p0) < 5e-3
    # one Adam step from identical weights: the updated head variables (sign-like Adam step) and the whole model must agree
    assert rel(k1, k0) < 2e-2 and rel(b1, b0) < 2e-2 and rel(f1, f0) < 2e-2


@pytest.mark.parametrize("B,H,W,Cin,Cout,k", [(2, 8, 8, 72, 64, 4), (1, 16, 16, 40, 32, 3), (2, 4, 4, 128, 128, 4), (1, 8, 16, 64, 24, 3)])
def test_quad_form_transposed_conv(gen, B, H, W, Cin, Cout, k):
    """Conv2DTranspose(k, strides 2, 'same') as tap-masked 3x3 convs on space-to-depth tensors (layers.QuadTConv,
    usseg_tconv_quad_fwd/dgrad/wgrad + usseg_space_to_depth2): forward, backward-data and weight gradient against the oracle."""
    from ultrasound_modeling_amd.layers import Conv2DTranspose, QuadTConv
    layer = Conv2DTranspose(Cin, Cout, k)
    w = rnd(gen, k, k, Cout, Cin, scale=1.0 / math.sqrt(k * k * Cin))
    b = rnd(gen, Cout, scale=0.5)
    layer.kernel.data.copy_(w); layer.bias.data.copy_(b)
    q = QuadTConv(layer)
    holder = torch.nn.ModuleList([layer])
    finalize(holder)
    q.on_finalize(torch.device(DEV))
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    ref = O.conv2d_transpose_s2_same(x, w, b)
    # forward: one stride-1 3x3 conv on the space-to-depth tensors; backward: the same kernel for backward data, the weight
    # gradient as tap-masked parity-class jobs of wgrad_halo (k=4) or the per-tap kernel (k=3), then the quad unpack
    wg = "wgrad_halo_kernel<2, 2, 2, true, 2, true>" if k == 4 else "wgrad_dma_kernel<1, 3>"
    y = on_route("conv_halo_kernel<1>", lambda: q.forward(xd))
    torch.cuda.synchronize()
    assert rel(y[..., :Cout], bf(ref)) < REL_BF16
    dy = rnd(gen, B, 2 * H, 2 * W, Cout)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xr, wr, b) * dy).sum().backward()
    dyd = to_dev_padded(dy)
    dx = on_route(("conv_halo_kernel<1>", wg, "tconv_quad_unpack_kernel"), lambda: q.backward(dyd))
    torch.cuda.synchronize()
    assert rel(dx[..., :Cin], bf(xr.grad)) < 2 * REL_BF16
    assert rel(layer.kernel.grad, wr.grad) < REL_F32
    assert rel(layer.bias.grad, dy.sum(dim=(0, 1, 2))) < REL_F32


@pytest.mark.parametrize("M,C", [(1, 3), (1000, 3), (16 * 128 * 128 + 5, 4), (77, 1)])
def test_accuracy_metric(gen, M, C):
    """usseg_accuracy == mean(argmax(probs) == argmax(y)) of TBI_ResNest.py:48-51, ties resolved to the first maximum as tf.argmax does."""
    from ultrasound_modeling_amd import ops
    probs = torch.rand(M, C, generator=gen).float()
    if M > 10:
        probs[3] = 0.25                      # an all-equal row: argmax 0
        probs[5, -1] = probs[5].max()        # a tie with the last class
    cls = torch.randint(0, C, (M,), generator=gen)
    y = torch.nn.functional.one_hot(cls, C).float()
    acc = torch.zeros(ops.ACC_FLOATS, device=DEV)
    a = ops.accuracy(probs.to(DEV), y.to(DEV), acc)
    ref = (probs.argmax(-1) == y.argmax(-1)).float().mean()
    assert abs(a.item() - ref.item()) < 1e-6
    a2 = ops.accuracy(probs.to(DEV), y.to(DEV), acc)          # the accumulator is reusable without zeroing
    assert a2.item() == a.item()


@pytest.mark.parametrize("M,C", [(300000, 3), (4099, 3)])
def test_accuracy_metric_four_pixels_per_trip(gen, M, C):
    """The three-class fast loop of usseg_accuracy (four pixels per thread and trip) with ties and a ragged tail."""
    from ultrasound_modeling_amd import ops
    probs = (torch.randint(0, 4, (M, C), generator=gen).float() / 4)        # many exact ties
    y = torch.nn.functional.one_hot(torch.randint(0, C, (M,), generator=gen), C).float()
    acc = torch.zeros(ops.ACC_FLOATS, device=DEV)
    a = ops.accuracy(probs.to(DEV), y.to(DEV), acc)
    ref = (probs.argmax(-1) == y.argmax(-1)).double().mean()
    assert abs(a.item() - ref.item()) < 1e-6


@pytest.mark.parametrize("n", [1, 255, 65536, 1000003])
def test_ordered_sum_of_a_loss_map(gen, n):
    """usseg_sum_f32 (the scalar of TBI_ResNest.py's [H,W] loss map): against the float64 sum, reusable accumulator, same bits on every call."""
    from ultrasound_modeling_amd import ops
    x = (torch.rand(n, generator=gen) * 3 - 1).float()
    acc = torch.zeros(ops.ACC_FLOATS, device=DEV)
    a = ops.sum_f32(x.to(DEV), acc).item()
    assert abs(a - x.double().sum().item()) <= 2e-6 * max(1.0, x.abs().double().sum().item())
    assert ops.sum_f32(x.to(DEV), acc).item() == a


# ------------------------------------------------------------------------------------------------ fused tile kernels vs the launches they replace
@pytest.mark.parametrize("cin,cv11,cvkk,oc", [(32, 3, 10, 64), (64, 7, 21, 128), (128, 14, 42, 256), (256, 28, 85, 512)])
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 8, 8), (3, 16, 5), (2, 4, 4), (1, 20, 36)])
def test_fused_cardinal_forward_equals_the_unfused_launches(gen, cin, cv11, cvkk, oc, B, H, W):
    """csrc/cardinal.hip on ragged geometries (the native 256x80 grid gives 64x20, 32x10, 16x5 stages; tiles are 8x8): every output of
    the fused launch against the six launches it replaces (same packed operands, same rounding points), incl. pad channels and the
    pooled partial rows.  Per-element bounds on seam data and a larger tile decode: test_gpu_fused_routes.py."""
    from ultrasound_modeling_amd import ops
    P = 3
    U, V = P * cv11, P * cvkk
    Up, Vp = (U + 7) // 8 * 8, (V + 7) // 8 * 8
    r16 = lambda n: (n + 15) // 16 * 16
    bfz = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).to(torch.bfloat16)
    x = bfz(B, H, W, cin).to(DEV)
    w1 = torch.zeros(r16(Up), cin, dtype=torch.bfloat16)
    w1[:U] = bfz(U, cin, sc=cin ** -0.5)
    w2 = torch.zeros(r16(Vp), 9 * Up, dtype=torch.bfloat16)
    for p_ in range(P):           # block diagonal: path p's outputs see only path p's inputs
        blk = bfz(cvkk, 9, cv11, sc=(9 * cv11) ** -0.5)
        for t in range(9):
            w2[p_ * cvkk:(p_ + 1) * cvkk, t * Up + p_ * cv11:t * Up + (p_ + 1) * cv11] = blk[:, t]
    wsc = bfz(oc, cin, sc=cin ** -0.5)
    padv = lambda n, np_, sc, off=0.0: torch.cat([off + sc * torch.randn(n, generator=gen), torch.zeros(np_ - n)]).to(DEV)
    b1, g1, be1 = padv(U, Up, 0.1), padv(U, Up, 0.2, 1.0), padv(U, Up, 0.1)
    b2, g2, be2 = padv(V, Vp, 0.1), padv(V, Vp, 0.2, 1.0), padv(V, Vp, 0.1)
    bsc, gsc, besc = padv(oc, oc, 0.1), padv(oc, oc, 0.2, 1.0), padv(oc, oc, 0.1)
    w1, w2, wsc = w1.to(DEV), w2.to(DEV), wsc.to(DEV)
    assert ops.cardinal_supported(cin, P, cv11, cvkk, Up, Vp, oc)
    u_raw, u, v_raw, y, gap, sc_raw, sc = ops.cardinal_fwd(x, w1, b1, g1, be1, w2, b2, g2, be2, wsc, bsc, gsc, besc, P, cv11, cvkk, Up, Vp, oc, 1e-3, 0.3)
    a = 0.3
    u_raw_u = ops.conv2d_fwd(x, w1, b1, 1, 1, ops.new_act(B, H, W, Up, DEV))
    u_u = ops.norm_act_fwd(u_raw_u, U, g1, be1, torch.empty_like(u_raw_u), 0, P, 1e-3, ops.ACT_LRELU, a)
    v_raw_u = ops.conv2d_fwd(u_u, w2, b2, 3, 1, ops.new_act(B, H, W, Vp, DEV))
    y_u = ops.norm_act_fwd(v_raw_u, V, g2, be2, torch.empty_like(v_raw_u), 0, P, 1e-3, ops.ACT_LRELU, a)
    sc_raw_u = ops.conv2d_fwd(x, wsc, bsc, 1, 1, ops.new_act(B, H, W, oc, DEV))
    sc_u = ops.norm_act_fwd(sc_raw_u, oc, gsc, besc, torch.empty_like(sc_raw_u), 0, 1, 1e-3, ops.ACT_LRELU, a)
    torch.cuda.synchronize()
    for nm, f_, u_ in (("u_raw", u_raw, u_raw_u), ("u", u, u_u), ("v_raw", v_raw, v_raw_u), ("y", y, y_u), ("sc_raw", sc_raw, sc_raw_u), ("sc", sc, sc_u)):
        assert rel(f_, u_) < REL_BF16, (nm, rel(f_, u_))
    for t, wlog in ((u_raw, U), (u, U), (v_raw, V), (y, V)):
        assert t.shape[3] == wlog or t[..., wlog:].abs().max().item() == 0
    pooled = gap[0].sum(dim=1)[:, :V] / (H * W)
    assert rel(pooled, y[..., :V].float().mean(dim=(1, 2))) < 1e-5


@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 16, 16), (2, 34, 18), (1, 64, 80), (3, 2, 6)])
def test_fused_stem_is_bit_identical_to_its_four_launches(gen, B, H, W):
    """csrc/stem.hip on ragged geometries (16x16 tiles, 3-pixel halo): y1, t1, the pre-norm convtmp_2 output and the pooled tensor are the
    BITS of conv1 + act -> convtmp_1 (+ shift) + act -> convtmp_2 -> BatchNorm + act + pool."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import BatchNormalization, Conv2D
    c1, c2, c3, bn = Conv2D(1, 16, 3), Conv2D(16, 32, 3), Conv2D(32, 32, 3), BatchNormalization(32)
    finalize(torch.nn.ModuleList([c1, c2, c3, bn]))
    f = lambda n, sc, off=0.0: (off + sc * torch.randn(n, generator=gen)).to(DEV)
    for c in (c1, c2, c3):
        c.bias.data.copy_(f(c.cout, 0.1))
        c.repack()
    bn.gamma.data.copy_(f(32, 0.2, 1.0)); bn.beta.data.copy_(f(32, 0.1))
    bn.moving_mean_p.copy_(f(32, 0.3)); bn.moving_variance_p.copy_(0.5 + torch.rand(32, generator=gen).to(DEV))
    shift = f(32, 0.1)
    x = torch.zeros(B, H, W, 8, dtype=torch.bfloat16)
    x[..., 0] = torch.randn(B, H, W, generator=gen).to(torch.bfloat16)
    x = x.to(DEV)
    y1, t1, cc, pooled = ops.stem_fwd(x, c1.wp_f, c1.bias.data, c2.wp_f, shift, c3.wp_f, c3.bias.data, bn.gamma.data, bn.beta.data,
                                      bn.moving_mean_p, bn.moving_variance_p, bn.eps, 0.3)
    y1u = c1.forward(x, act=ops.ACT_LRELU, alpha=0.3)
    t1u = c2.forward(y1u, act=ops.ACT_LRELU, alpha=0.3, bias=shift)
    ccu = c3.forward(t1u)
    pu = bn.forward_pool(ccu, ops.ACT_LRELU, 0.3)
    torch.cuda.synchronize()
    for nm, f_, u_ in (("y1", y1, y1u), ("t1", t1, t1u), ("c2", cc, ccu), ("pooled", pooled, pu)):
        assert torch.equal(f_, u_), (nm, rel(f_, u_))


@pytest.mark.parametrize("cin,cv11,cvkk,oc", [(32, 3, 10, 64), (64, 7, 21, 128), (128, 14, 42, 256), (256, 28, 85, 512)])
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 8, 8), (3, 16, 5), (2, 4, 4), (1, 20, 36)])
def test_fused_cardinal_backward_equals_the_unfused_launches(gen, cin, cv11, cvkk, oc, B, H, W):
    """csrc/cardinal.hip backward (K3) on ragged geometries: dv, du_raw, dsc_raw and the nine per-channel gradient vectors of the ONE fused
    launch against the four launches it replaces (norm_act_bwd_sa -> conv2d_dgrad 3x3 -> norm_act_bwd | norm_act_bwd of the shortcut) on the
    same inputs and packed operands; same rounding points (dv and du are bf16 where the unfused launches store them).  Per-element bounds
    and the persistent walk (more tiles than workgroup pairs): test_gpu_fused_routes.py."""
    from ultrasound_modeling_amd import ops
    P = 3
    U, V = P * cv11, P * cvkk
    Up, Vp = (U + 7) // 8 * 8, (V + 7) // 8 * 8
    r16 = lambda n: (n + 15) // 16 * 16
    bfz = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).to(torch.bfloat16)

    def padded(n, npad, *lead, sc=1.0):
        t = torch.zeros(*lead, npad, dtype=torch.bfloat16)
        t[..., :n] = bfz(*lead, n, sc=sc)
        return t.to(DEV)
    v_raw, dout = padded(V, Vp, B, H, W), padded(V, Vp, B, H, W)
    u_raw = padded(U, Up, B, H, W)
    sc_raw, dsc = bfz(B, H, W, oc).to(DEV), bfz(B, H, W, oc).to(DEV)
    w2d = torch.zeros(r16(Up), 9 * Vp, dtype=torch.bfloat16)
    for p_ in range(P):           # block diagonal backward-data operand: rows = the path's inputs, K = (tap, the path's outputs)
        blk = bfz(cv11, 9, cvkk, sc=(9 * cvkk) ** -0.5)
        for t in range(9):
            w2d[p_ * cv11:(p_ + 1) * cv11, t * Vp + p_ * cvkk:t * Vp + (p_ + 1) * cvkk] = blk[:, t]
    w2d = w2d.to(DEV)
    padv = lambda n, np_, sc, off=0.0: torch.cat([off + sc * torch.randn(n, generator=gen), torch.zeros(np_ - n)]).to(DEV)
    g1, be1 = padv(U, Up, 0.2, 1.0), padv(U, Up, 0.1)
    g2, be2 = padv(V, Vp, 0.2, 1.0), padv(V, Vp, 0.1)
    gsc, besc = padv(oc, oc, 0.2, 1.0), padv(oc, oc, 0.1)
    sa_s = torch.rand(B, V, generator=gen).to(DEV)
    sa_dg = (0.05 * torch.randn(B, V, generator=gen)).to(DEV)
    a, mult = 0.3, 3.0
    z = lambda n: torch.zeros(n, device=DEV)
    gf = [z(Vp), z(Vp), z(Vp), z(Up), z(Up), z(Up), z(oc), z(oc), z(oc)]
    dv = ops.new_act(B, H, W, Vp, DEV)
    dcat = ops.new_act(B, H, W, Up + oc, DEV)
    ops.cardinal_bwd(dout, dsc, v_raw, u_raw, sc_raw, w2d, g2, be2, g1, be1, gsc, besc, sa_s, sa_dg, mult, dv, dcat, gf, cin, P, cv11, cvkk, Up, Vp, oc,
                     1e-3, a)
    gu = [z(Vp), z(Vp), z(Vp), z(Up), z(Up), z(Up), z(oc), z(oc), z(oc)]
    dv_u = ops.norm_act_bwd_sa(v_raw, dout, V, g2, be2, torch.empty_like(v_raw), gu[0], gu[1], 0, P, 1e-3, ops.ACT_LRELU, a, sa_s, sa_dg, mult, dbias=gu[2])
    du_u = ops.conv2d_dgrad(dv_u, w2d, 3, 1, torch.empty_like(u_raw))
    dur_u = ops.norm_act_bwd(u_raw, du_u, U, g1, be1, torch.empty_like(u_raw), gu[3], gu[4], 0, P, 1e-3, ops.ACT_LRELU, a, dbias=gu[5])
    dsr_u = ops.norm_act_bwd(sc_raw, dsc, oc, gsc, besc, torch.empty_like(sc_raw), gu[6], gu[7], 0, 1, 1e-3, ops.ACT_LRELU, a, dbias=gu[8])
    torch.cuda.synchronize()
    assert rel(dv, dv_u) < REL_BF16, ("dv", rel(dv, dv_u))
    assert rel(dcat[..., :Up], dur_u) < 2 * REL_BF16, ("du_raw", rel(dcat[..., :Up], dur_u))      # behind two bf16 storage points (dv, du)
    assert rel(dcat[..., Up:], dsr_u) < REL_BF16, ("dsc_raw", rel(dcat[..., Up:], dsr_u))
    assert Vp == V or dv[..., V:].abs().max().item() == 0
    assert Up == U or dcat[..., U:Up].abs().max().item() == 0
    names = ("dgamma2", "dbeta2", "dbias2", "dgamma1", "dbeta1", "dbias1", "dgamma_sc", "dbeta_sc", "dbias_sc")
    for nm, f_, u_ in zip(names, gf, gu):
        assert rel(f_, u_) < (2e-3 if "1" in nm else 1e-4), (nm, rel(f_, u_))


@pytest.mark.parametrize("oc,cvkk,B,H,W", [(64, 10, 2, 128, 128), (128, 21, 4, 96, 96), (64, 10, 1, 64, 64)])
def test_paired_layernorm_backward_is_the_bits_of_the_two_launches(gen, oc, cvkk, B, H, W):
    """usseg_norm_act_bwd_pair (the shortcut norm's backward and conv2_bn's backward with the re-weighting folded in, one launch, two workgroup
    roles on the same tile loop) against the two launches it replaces: dx tensors and the six gradient vectors are bit-identical; a pair without
    an instantiation (here: fewer than 32k pixels) reports False and launches nothing."""
    from ultrasound_modeling_amd import ops
    P, V = 3, 3 * cvkk
    Vp = (V + 7) // 8 * 8
    bfz = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16)
    xa, dya = bfz(B, H, W, oc).to(DEV), bfz(B, H, W, oc).to(DEV)
    xb = torch.zeros(B, H, W, Vp, dtype=torch.bfloat16)
    xb[..., :V] = bfz(B, H, W, V)
    db_ = torch.zeros(B, H, W, Vp, dtype=torch.bfloat16)
    db_[..., :V] = bfz(B, H, W, V)
    xb, db_ = xb.to(DEV), db_.to(DEV)
    padv = lambda n, np_, sc, off=0.0: torch.cat([off + sc * torch.randn(n, generator=gen), torch.zeros(np_ - n)]).to(DEV)
    ga, ba, gb, bb = padv(oc, oc, 0.2, 1.0), padv(oc, oc, 0.1), padv(V, Vp, 0.2, 1.0), padv(V, Vp, 0.1)
    sa_s, sa_dg = torch.rand(B, V, generator=gen).to(DEV), (0.05 * torch.randn(B, V, generator=gen)).to(DEV)
    z = lambda n: torch.zeros(n, device=DEV)
    gp = [z(oc), z(oc), z(oc), z(Vp), z(Vp), z(Vp)]
    dxa, dxb = torch.empty_like(xa), torch.empty_like(xb)
    took = ops.norm_act_bwd_pair(xa, dya, oc, ga, ba, dxa, gp[0], gp[1], gp[2], xb, db_, V, P, gb, bb, dxb, gp[3], gp[4], gp[5], sa_s, sa_dg, 3.0, 1e-3, 0.3)
    if B * H * W < 32768:
        assert not took
        return
    assert took
    gu = [z(oc), z(oc), z(oc), z(Vp), z(Vp), z(Vp)]
    dxa_u = ops.norm_act_bwd(xa, dya, oc, ga, ba, torch.empty_like(xa), gu[0], gu[1], 0, 1, 1e-3, ops.ACT_LRELU, 0.3, dbias=gu[2])
    dxb_u = ops.norm_act_bwd_sa(xb, db_, V, gb, bb, torch.empty_like(xb), gu[3], gu[4], 0, P, 1e-3, ops.ACT_LRELU, 0.3, sa_s, sa_dg, 3.0, dbias=gu[5])
    torch.cuda.synchronize()
    assert torch.equal(dxa, dxa_u) and torch.equal(dxb, dxb_u)
    for f_, u_ in zip(gp, gu):
        assert rel(f_, u_) < 1e-5        # (the partial rows are summed over a different number of workgroups)


@pytest.mark.parametrize("B,H,W,Cin,q", [(2, 64, 64, 64, 16), (1, 128, 128, 128, 16), (2, 32, 48, 32, 16)])
def test_streaming_conv_jobs_of_one_plan_in_one_launch(gen, monkeypatch, B, H, W, Cin, q):
    """conv_stream with blockIdx.z = job (the three dilation branches of a decoder stage whose weights fit in LDS): the merged launch gives
    the bits of one launch per job (USSEG_STREAM_MERGE=0), and both agree with the fp64 oracle."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    dil = (2, 4, 8)
    holder, ws, bs = torch.nn.ModuleList(), [], []
    for j in range(3):
        c = Conv2D(Cin, q, 3, dil[j])
        w = rnd(gen, 3, 3, Cin, q, scale=1.0 / math.sqrt(9 * Cin))
        b = rnd(gen, q, scale=0.5)
        c.kernel.data.copy_(w); c.bias.data.copy_(b)
        holder.append(c); ws.append(w); bs.append(b)
    finalize(holder)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("USSEG_STREAM_MERGE", flag)
        out = torch.zeros(B, H, W, 3 * q, dtype=torch.bfloat16, device=DEV)
        ops.conv2d_fwd_multi([(xd, c.wp_f, c.bias.data, c.k, c.dil, out[..., j * q:(j + 1) * q], ops.ACT_LRELU, 0.3) for j, c in enumerate(holder)])
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    for j in range(3):
        ref = torch.nn.functional.leaky_relu(O.conv2d_same(x, ws[j], bs[j], dil[j]), 0.3)
        assert rel(outs[0][..., j * q:(j + 1) * q], bf(ref)) < REL_BF16, j


@pytest.mark.parametrize("B,H,W,Cin,q", [(2, 32, 32, 64, 16), (1, 64, 48, 128, 16), (2, 32, 32, 512, 64), (3, 16, 16, 256, 32), (1, 128, 128, 72, 16), (2, 64, 64, 40, 24)])
def test_one_by_one_branch_as_fourth_job_of_the_dilated_launch(gen, monkeypatch, B, H, W, Cin, q):
    """The DecoderBlock's 1x1 branch as a centre-tap-only job of the three dilated 3x3 convs' multi-job launch (conv_big / conv_stream
    `one_tap`, Decoder.py:61-66): every branch against the fp64 oracle, the dilated branches bit-identical to the three-job launch, and the
    1x1 branch against its own launch (another kernel with another K chunking: bf16-level agreement)."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    dil = (1, 2, 4, 8)
    holder, ws, bs = torch.nn.ModuleList(), [], []
    for j in range(4):
        k = 1 if j == 0 else 3
        c = Conv2D(Cin, q, k, dil[j])
        w = rnd(gen, k, k, Cin, q, scale=1.0 / math.sqrt(k * k * Cin))
        b = rnd(gen, q, scale=0.5)
        c.kernel.data.copy_(w); c.bias.data.copy_(b)
        holder.append(c); ws.append(w); bs.append(b)
    finalize(holder)
    x = rnd(gen, B, H, W, Cin)
    xd = to_dev_padded(x)
    job = lambda out, j: (xd, holder[j].wp_f, holder[j].bias.data, holder[j].k, holder[j].dil, out[..., j * q:(j + 1) * q], ops.ACT_LRELU, 0.3)
    out4 = torch.zeros(B, H, W, 4 * q, dtype=torch.bfloat16, device=DEV)
    ops.conv2d_fwd_multi([job(out4, j) for j in range(4)])
    out3 = torch.zeros_like(out4)
    ops.conv2d_fwd(xd, holder[0].wp_f, holder[0].bias.data, 1, 1, out3[..., :q], ops.ACT_LRELU, 0.3)
    ops.conv2d_fwd_multi([job(out3, j) for j in (1, 2, 3)])
    torch.cuda.synchronize()
    assert torch.equal(out4[..., q:], out3[..., q:])
    assert rel(out4[..., :q], out3[..., :q]) < REL_BF16
    for j in range(4):
        ref = torch.nn.functional.leaky_relu(O.conv2d_same(x, ws[j], bs[j], dil[j]), 0.3)
        assert rel(out4[..., j * q:(j + 1) * q], bf(ref)) < REL_BF16, j


@pytest.mark.parametrize("B,h,w,C,k,cin", [(2, 32, 32, 3, 3, 72), (1, 20, 36, 3, 3, 16), (3, 16, 5, 3, 3, 72), (2, 48, 16, 2, 4, 40), (1, 64, 64, 4, 3, 16)])
def test_fused_quad_head_softmax_loss_equals_its_three_launches(gen, B, h, w, C, k, cin):
    """usseg_head_quad_softmax_loss (quad-form head conv + bias + softmax + CategoricalCrossentropy + d loss / d logits in one launch) against
    usseg_quad_bias_expand + usseg_conv2d_fwd (fp32 quad logits) + usseg_softmax_loss_fwd_bwd on ragged sizes, and the probabilities against
    the fp64 oracle's transposed conv + softmax."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2DTranspose, QuadHead
    head = Conv2DTranspose(cin, C, k)
    q = QuadHead(head)
    finalize(head)
    wk = rnd(gen, k, k, C, cin, scale=1.0 / math.sqrt(k * k * cin))
    bk = rnd(gen, C, scale=0.5)
    head.kernel.data.copy_(wk); head.bias.data.copy_(bk)
    q.on_finalize(DEV)
    x = rnd(gen, B, h, w, cin)
    xd = to_dev_padded(x)
    y = torch.softmax(torch.randn(B, 2 * h, 2 * w, C, generator=gen), -1).to(DEV)
    inv = 1.0 / 7.0
    # unfused
    logits = q.forward(xd)
    probs_u = torch.empty(B, 2 * h, 2 * w, C, device=DEV)
    loss_u = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl_u = ops.new_act(B, h, w, 16, DEV)
    ops.softmax_loss(logits, y, probs_u, loss_u, dl_u, HW=4 * h * w, C_classes=C, loss_kind=0, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=inv,
                     quad_w=2 * w)
    # fused
    probs_f = torch.empty_like(probs_u)
    loss_f = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl_f = ops.new_act(B, h, w, 16, DEV)
    took = q.forward_loss(xd, y, probs_f, loss_f, dl_f, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=inv)
    if xd.shape[-1] not in (16, 72):
        assert not took           # no instantiation for this input width: nothing launched, the caller runs the three launches
        return
    assert took
    probs_n = torch.empty_like(probs_u)
    assert q.forward_loss(xd, None, probs_n, None, None)            # probabilities only
    torch.cuda.synchronize()
    assert rel(probs_f, probs_u) < 1e-5 and torch.equal(probs_n, probs_f)
    assert abs(loss_f[0].item() - loss_u[0].item()) < 1e-5 * abs(loss_u[0].item())
    assert rel(dl_f, dl_u) < REL_BF16
    if C < 4:
        assert dl_f.reshape(B, h, w, 4, 4)[..., C:].abs().max().item() == 0          # the pad classes of every parity slot
    ref = torch.softmax(O.conv2d_transpose_s2_same(x, wk, bk), -1)
    assert rel(probs_f, ref) < 2e-3


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (1, 20, 36), (3, 16, 5), (1, 64, 48)])
@pytest.mark.parametrize("mode", [2, 0])
def test_fused_stem_dgrad_with_the_backward_in_front_of_it(gen, mode, B, H, W):
    """usseg_conv3_dgrad_actbwd (csrc/stem.hip): a stem conv's backward-data pass + folded-BatchNorm / LeakyReLU backward (mode 2, 32 channels) or
    LeakyReLU backward + column sums (mode 0, 16 channels) in one launch against the two launches it replaces (usseg_conv2d_dgrad, then
    usseg_norm_act_bwd mode 2 / usseg_act_bwd_colsum), on ragged sizes.  The fused form keeps the intermediate gradient in fp32 where the pair
    stores it in bf16, so both are also held against a float64 restatement of the chain."""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.layers import Conv2D
    co = 32 if mode == 2 else 16
    conv = Conv2D(co, 32, 3)
    finalize(conv)
    conv.kernel.data.copy_(rnd(gen, 3, 3, co, 32, scale=1.0 / math.sqrt(9 * co)))
    conv.repack()
    dy = to_dev_padded(rnd(gen, B, H, W, 32))
    yact = to_dev_padded(rnd(gen, B, H, W, co))                      # the stored activated output of the layer in front (any sign)
    f = lambda n, sc, off=0.0: (off + sc * torch.randn(n, generator=gen)).to(DEV)
    gamma, beta, var = f(co, 0.2, 1.0), f(co, 0.1), (0.5 + torch.rand(co, generator=gen)).to(DEV)
    mean = f(co, 0.1)
    z = lambda: torch.zeros(co, device=DEV)
    dgf, dbf, dbif = z(), z(), z()
    dxf = torch.empty_like(yact)
    if mode == 2:
        took = ops.conv3_dgrad_actbwd(dy, conv.wp_d, yact, dxf, 2, 0.3, dbif, gamma, beta, var, 1e-3, dgf, dbf)
    else:
        took = ops.conv3_dgrad_actbwd(dy, conv.wp_d, yact, dxf, 0, 0.3, dbif)
    assert took
    din = ops.conv2d_dgrad(dy, conv.wp_d, 3, 1, torch.empty_like(yact))
    dgu, dbu, dbiu = z(), z(), z()
    if mode == 2:
        dxu = ops.norm_act_bwd(yact, din, co, gamma, beta, torch.empty_like(yact), dgu, dbu, 2, 1, 1e-3, ops.ACT_LRELU, 0.3, mean, var, dbias=dbiu)
    else:
        dxu = ops.act_bwd_colsum(yact, din, torch.empty_like(yact), ops.ACT_LRELU, 0.3, dbiu, co)
    torch.cuda.synchronize()
    # float64 restatement of the chain on the same bf16 inputs: the fused launch (fp32 intermediate) sits well inside the bar, the pair (bf16
    # intermediate: 2^-9 per element, which a sum over random signs does not average away) only just; fused against pair at the pair's noise
    F = torch.nn.functional
    w64 = conv.kernel.detach().to(torch.bfloat16).double().cpu().permute(3, 2, 0, 1)                  # [32, co, 3, 3]
    d64 = F.conv_transpose2d(dy[..., :32].double().cpu().permute(0, 3, 1, 2), w64, padding=1).permute(0, 2, 3, 1)
    y64 = yact[..., :co].double().cpu()
    if mode == 2:
        g64, b64, r64 = gamma.double().cpu(), beta.double().cpu(), (var.double().cpu() + 1e-3).rsqrt()
        dh = d64 * torch.where(y64 > 0, 1.0, 0.3)
        xh = (torch.where(y64 >= 0, y64, y64 / 0.3) - b64) / g64
        dx64 = dh * g64 * r64
        refs = {"dgamma": ((dh * xh).sum((0, 1, 2)), dgf, dgu), "dbeta": (dh.sum((0, 1, 2)), dbf, dbu), "dbias": (dx64.sum((0, 1, 2)), dbif, dbiu)}
    else:
        dx64 = d64 * torch.where(y64 >= 0, 1.0, 0.3)
        refs = {"dbias": (dx64.to(torch.bfloat16).double().sum((0, 1, 2)), dbif, dbiu)}      # usseg_act_bwd_colsum sums the STORED values
    assert rel(dxf[..., :co], dx64) < 3e-3, rel(dxf[..., :co], dx64)
    assert rel(dxf, dxu) < 4e-3, rel(dxf, dxu)
    for name, (r64_, fused, pair) in refs.items():
        assert rel(fused, r64_) < 1.5e-3, (name, rel(fused, r64_))
        assert rel(fused, pair) < 4e-3, (name, rel(fused, pair))
