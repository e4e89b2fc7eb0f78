"""Conv route matrix (GPU): every conv kernel route, the kernel each case lands on, and a per-element error bound.

Each case first asserts WHICH kernel the pass launched (route_probe.routed: torch.profiler device activity), then checks every
output element against the fp64 oracle with |y - ref| <= c*u*(|x| (*) |w|) + tiny (route_probe.assert_elementwise), pad
channels for exact zeros and the elements outside channel-slice views for being untouched.  Routes are driven by shapes and
by the knobs the planners read on every call (USSEG_STREAM_MIN_STEPS, USSEG_STREAM_WGX, USSEG_STREAM_MERGE, USSEG_BIG_W8,
USSEG_TCONV_HALO); knobs cached once per process are never used.

Inputs carry one rare large element (x64) and, in the last image, rows that are non-zero only next to the 16-row tile
seams and at the bottom edge: an error confined to one tile seam, one pixel group or the ragged tail is not averaged away.
Large shapes are checked over row bands (every 16-row seam in the last 48 rows, the middle seam, the first and last rows
of the first and last image) with the same fp64 oracle on a cropped input.

Routes that no shape reaches under the current thresholds (listed, not forced through cached knobs):
  * igemm_dma_kernel<8, 3>: only with USSEG_IGEMM_STAGES8=3 (cached); the planner's 128-channel tiles use 2 or 4 stages.
  * the npatches < 2^20 guards of big_fill_job and wgrad_halo: the pixel guard always binds first (see CONV_LIMITS).
Routes reached only past a size guard, tested there: igemm_kernel<NT, 8> (K step 64; test_limit_edge_igemm) and the non-DMA
wgrad_kernel (test_limit_edge_wgrad, test_batched_gemm_tn_route).  Forward passes of the size guards are checked over row bands;
the weight gradients past them against an fp64 reduction taken on the device.
The `fast_wait` argument of conv_stream_kernel is not part of the kernel name: the cases below cover both values (Cout a
multiple of the channel tile and not, with and without residual), but the probe cannot tell which one a launch used.
The quad-form transposed conv, the tconv parity-class forms and the deferred weight-gradient finish are route-checked in
test_gpu_ops.py, beside their existing parity tests.
"""
import math

import pytest
import torch

import usseg_oracle as O
from route_probe import U_BF16, U_F32, assert_elementwise, bf, c_f32, routed, seam_data, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA = 0.3


def rows_checked(B, H, force=False):
    """(image, row) pairs the banded check covers: everything for small tensors."""
    if B * H <= 256 and not force:
        return None
    rows = {0, 1, H // 2 - 1, H // 2, H - 1, H - 2}
    for s in range(max(0, H - 48) // 16 * 16, H, 16):
        rows.update({s - 1, s})
    rows = sorted(r for r in rows if 0 <= r < H)
    return [(b, rows) for b in sorted({0, B - 1})]


def banded(f, x, pad, bands):
    """f(crop of x) restricted to the bands: f is a stride-1 'SAME' op with a `pad`-row reach."""
    if bands is None:
        return f(x)
    outs = []
    H = x.shape[1]
    for b, rows in bands:
        for r in rows:
            lo, hi = max(0, r - pad), min(H, r + pad + 1)
            outs.append(f(x[b:b + 1, lo:hi])[:, r - lo])
    return torch.cat(outs)


def pick(y, bands):
    if bands is None:
        return y
    return torch.cat([y[b:b + 1, r] for b, rows in bands for r in rows])


def make_conv(gen, Cin, Cout, k, dil):
    from ultrasound_modeling_amd.flat import FlatParams
    from ultrasound_modeling_amd.layers import Conv2D
    layer = Conv2D(Cin, Cout, k, dil)
    w = bf(torch.randn(k, k, Cin, Cout, generator=gen, dtype=torch.float64) / math.sqrt(k * k * Cin))
    b = bf(torch.randn(Cout, generator=gen, dtype=torch.float64) * 0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    FlatParams(layer, DEV)
    return layer, w, b


def act_ref(v, epi):
    if epi == "lrelu" or epi == "res":
        return torch.where(v >= 0, v, ALPHA * v)
    if epi == "elu":
        return torch.where(v > 0, v, torch.expm1(v.clamp(max=0)))
    return v


# ------------------------------------------------------------------------------------------------ forward
# (id, (B, H, W, Cin, Cout, dil), env, epilogue, expected kernel)
FWD = [
    # conv_stream: NS 4 (256-pixel tiles) / NS 2 (128), NT 1 / 2 / 4, residual variant, Cout on / off the channel tile (fast_wait)
    ("stream_ns4_nt2", (2, 16, 16, 16, 32, 1), {}, "lrelu", "conv_stream_kernel<2, 4, false>"),
    ("stream_ns4_nt2_res", (2, 16, 16, 16, 32, 1), {}, "res", "conv_stream_kernel<2, 4, true>"),
    ("stream_ns4_nt1", (1, 64, 64, 8, 16, 1), {}, "bias", "conv_stream_kernel<1, 4, false>"),
    ("stream_ns4_nt1_res", (1, 64, 64, 8, 16, 1), {}, "res", "conv_stream_kernel<1, 4, true>"),
    ("stream_ns4_nt4", (3, 16, 16, 24, 136, 1), {}, "elu", "conv_stream_kernel<4, 4, false>"),
    ("stream_ns4_nt4_res", (3, 16, 16, 24, 136, 1), {}, "res", "conv_stream_kernel<4, 4, true>"),
    ("stream_ns2_nt2", (1, 8, 16, 64, 32, 1), {}, "lrelu", "conv_stream_kernel<2, 2, false>"),
    ("stream_ns2_nt2_res", (1, 8, 16, 64, 32, 1), {}, "res", "conv_stream_kernel<2, 2, true>"),
    ("stream_ns2_nt1", (2, 8, 16, 16, 16, 1), {}, "bias", "conv_stream_kernel<1, 2, false>"),
    ("stream_ns2_nt4", (4, 256, 256, 8, 64, 1), {"USSEG_STREAM_MIN_STEPS": "4"}, "bias", "conv_stream_kernel<4, 2, false>"),
    ("stream_no_fast_wait", (5, 32, 64, 16, 40, 1), {"USSEG_STREAM_MIN_STEPS": "1", "USSEG_STREAM_WGX": "16"}, "lrelu", "conv_stream_kernel<4, 4, false>"),
    ("stream_many_steps", (1, 128, 128, 32, 32, 4), {"USSEG_STREAM_MIN_STEPS": "1", "USSEG_STREAM_WGX": "8"}, "lrelu", "conv_stream_kernel<2, 4, false>"),
    ("stream_view", (2, 16, 16, 16, 24, 1), {}, "view", "conv_stream_kernel<2, 4, false>"),
    # conv_big: 128-pixel tiles on four waves, 256-pixel tiles on eight (forced per call and chosen by the planner)
    ("big_128", (1, 128, 128, 64, 64, 1), {}, "lrelu", "conv_big_kernel<1, 2, 4>"),
    ("big_128_f32", (2, 256, 256, 64, 16, 4), {}, "f32", "conv_big_kernel<1, 2, 4>"),
    ("big_128_res", (1, 128, 128, 64, 64, 1), {}, "res", "conv_big_kernel<1, 2, 4>"),
    ("big_128_scale", (1, 128, 128, 64, 64, 1), {}, "scale", "conv_big_kernel<1, 2, 4>"),
    ("big_w8_forced", (1, 128, 128, 64, 64, 1), {"USSEG_BIG_W8": "2"}, "lrelu", "conv_big_kernel<1, 2, 8>"),
    ("big_w8_f32", (4, 128, 128, 64, 64, 2), {}, "f32", "conv_big_kernel<4, 2, 8>"),
    ("big_256", (8, 256, 256, 64, 64, 1), {}, "lrelu", "conv_big_kernel<4, 4, 4>"),
    ("big_view", (1, 128, 128, 64, 56, 1), {}, "view", "conv_big_kernel<1, 2, 4>"),
    # conv_halo: NT 1 / 2 / 4 tiles, lattices of dilation 2 / 4 / 8
    ("halo_nt1", (2, 32, 32, 64, 64, 8), {}, "lrelu", "conv_halo_kernel<1>"),
    ("halo_nt1_f32", (2, 16, 16, 16, 32, 1), {}, "f32", "conv_halo_kernel<1>"),
    ("halo_nt2_f32", (2, 128, 128, 16, 32, 1), {}, "f32", "conv_halo_kernel<2>"),
    ("halo_nt4_f32", (2, 128, 128, 32, 64, 2), {}, "f32", "conv_halo_kernel<4>"),
    ("halo_res", (2, 16, 16, 72, 136, 2), {}, "res", "conv_halo_kernel<1>"),
    ("halo_elu", (3, 16, 16, 96, 40, 4), {}, "elu", "conv_halo_kernel<1>"),
    ("halo_scale", (2, 16, 16, 16, 32, 1), {}, "scale", "conv_halo_kernel<1>"),
    ("halo_view", (2, 32, 32, 48, 24, 4), {}, "view", "conv_halo_kernel<1>"),
    # conv_halo_persist: the planner sends the plain bf16 pass to conv_stream; the out_f32 / scale passes and a too-short stream
    # walk (USSEG_STREAM_MIN_STEPS, read per call) reach it
    ("persist_nt2_f32", (2, 256, 256, 16, 32, 1), {}, "f32", "conv_halo_persist_kernel<2>"),
    ("persist_nt1_f32", (5, 256, 128, 24, 8, 2), {}, "f32", "conv_halo_persist_kernel<1>"),
    ("persist_nt4_f32", (8, 128, 128, 32, 64, 1), {}, "f32", "conv_halo_persist_kernel<4>"),
    ("persist_nt2_scale", (2, 256, 256, 16, 32, 1), {}, "scale", "conv_halo_persist_kernel<2>"),
    ("persist_nt2_bf16", (2, 256, 256, 16, 32, 1), {"USSEG_STREAM_MIN_STEPS": "1000000"}, "lrelu", "conv_halo_persist_kernel<2>"),
    ("persist_lattice8", (8, 256, 64, 16, 32, 8), {}, "lrelu", "conv_halo_persist_kernel<2>"),      # by shape: 8-wide lattices
    ("persist_lattice8_view", (8, 256, 64, 16, 24, 8), {}, "view", "conv_halo_persist_kernel<2>"),
    ("persist_nt2_res", (2, 256, 256, 16, 32, 1), {"USSEG_STREAM_MIN_STEPS": "1000000"}, "res", "conv_halo_persist_kernel<2>"),
    # gather GEMMs (1x1): igemm (K step 32), igemm_dma NT 1 / 2 / 4 / 8 with 3 / 2 / 4 stages, the persistent form
    ("igemm_kc4", (3, 7, 5, 16, 24, 1), {}, "lrelu", "igemm_kernel<2, 4>"),
    ("igemm_kc4_f32", (1, 6, 10, 24, 8, 1), {}, "f32", "igemm_kernel<1, 4>"),
    ("igemm_dma_nt1", (1, 6, 10, 40, 8, 1), {}, "lrelu", "igemm_dma_kernel<1, 3>"),
    ("igemm_dma_nt2", (3, 9, 7, 136, 32, 1), {}, "res", "igemm_dma_kernel<2, 3>"),
    ("igemm_dma_nt4", (8, 64, 64, 64, 64, 1), {}, "f32", "igemm_dma_kernel<4, 3>"),
    ("igemm_dma_nt8_2st", (2, 128, 128, 64, 128, 1), {}, "f32", "igemm_dma_kernel<8, 2>"),
    ("igemm_dma_nt8_4st", (2, 128, 128, 512, 128, 1), {}, "scale", "igemm_dma_kernel<8, 4>"),
    ("igemm_dma_view", (2, 12, 12, 1024, 40, 1), {}, "view", "igemm_dma_kernel<2, 3>"),
    ("igemm_dma_persist", (8, 128, 128, 32, 16, 1), {}, "lrelu", "igemm_dma_persist_kernel<1, 3>"),
    ("igemm_dma_persist_nt4", (8, 128, 128, 40, 64, 1), {}, "elu", "igemm_dma_persist_kernel<4, 3>"),
]


def _fwd_case(gen, monkeypatch, shape, env, epi, expect, k=None):
    from ultrasound_modeling_amd import ops
    B, H, W, Cin, Cout, dil = shape
    k = k or (1 if expect.startswith("igemm") else 3)
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    layer, w, b = make_conv(gen, Cin, Cout, k, dil)
    x = seam_data(gen, B, H, W, Cin)
    bands = rows_checked(B, H)
    pad = dil * (k // 2)
    kw = dict(act=ops.ACT_NONE)
    r = None
    sc = None
    if epi in ("lrelu", "res"):
        kw = dict(act=ops.ACT_LRELU, alpha=ALPHA)
    elif epi == "elu":
        kw = dict(act=ops.ACT_ELU, alpha=1.0)
    if epi == "res":
        r = seam_data(gen, B, H, W, Cout)
        kw["residual"] = to_dev(r)[1]
    if epi == "f32":
        kw["out_f32"] = True
    if epi == "scale":
        sc = bf(torch.rand(Cout, generator=gen, dtype=torch.float64) + 0.5)
        scd = torch.zeros(layer.cout_p, dtype=torch.float32, device=DEV)
        shd = torch.zeros(layer.cout_p, dtype=torch.float32, device=DEV)
        scd[:Cout] = sc.float().to(DEV)
        shd[:Cout] = b.float().to(DEV)
        kw.update(scale=scd, shift=shd)
    if epi == "view":
        xbuf, xd = to_dev(x, ld=layer.cin_p + 16, off=8, fill=5.0)
        ybuf = torch.full((B, H, W, layer.cout_p + 24), -3.0, dtype=torch.bfloat16, device=DEV)
        kw["out"] = ybuf[..., 16:16 + layer.cout_p]
    else:
        xd = to_dev(x)[1]
    y, _ = routed(lambda: layer.forward(xd, **kw), expect)
    torch.cuda.synchronize()
    ws = w if sc is None else w * sc
    f = lambda xx: O.conv2d_same(xx, ws, b, dil)
    fm = lambda xx: O.conv2d_same(xx.abs(), ws.abs(), b.abs(), dil)
    ref, mag = act_ref(banded(f, x, pad, bands), epi), banded(fm, x, pad, bands)
    if r is not None:
        ref, mag = ref + pick(r, bands), mag + pick(r.abs(), bands)
    u, c = (U_F32, c_f32(k * k * Cin)) if epi == "f32" else (U_BF16, 4.0)
    assert_elementwise(pick(y[..., :Cout], bands), ref, mag, u, c, what=f"forward {expect}")
    if epi != "f32" and layer.cout_p > Cout:
        assert y[..., Cout:].abs().max().item() == 0, "pad channels"
    if epi == "view":
        assert (ybuf[..., :16] == -3.0).all() and (ybuf[..., 16 + layer.cout_p:] == -3.0).all(), "outside the output view"
        assert (xbuf[..., :8] == 5.0).all() and (xbuf[..., 8 + layer.cin_p:] == 5.0).all(), "input buffer"


@pytest.mark.parametrize("shape,env,epi,expect", [c[1:] for c in FWD], ids=[c[0] for c in FWD])
def test_forward_route(gen, monkeypatch, shape, env, epi, expect):
    _fwd_case(gen, monkeypatch, shape, env, epi, expect)


@pytest.fixture(scope="module")
def gen():
    return torch.Generator().manual_seed(4321)


# ------------------------------------------------------------------------------------------------ backward data
# (id, (B, H, W, Cin, Cout, dil), env, epilogue, expected kernel); epilogue: plain / accumulate / res / view
DGRAD = [
    ("stream_ns4_nt1", (2, 16, 16, 16, 32, 1), {}, "plain", "conv_stream_kernel<1, 4, false>"),
    ("stream_ns4_nt4", (1, 32, 32, 64, 16, 2), {}, "plain", "conv_stream_kernel<4, 4, false>"),
    ("stream_ns4_nt2", (5, 256, 128, 24, 8, 2), {}, "plain", "conv_stream_kernel<2, 4, false>"),
    ("stream_ns2_nt4", (1, 8, 16, 64, 32, 1), {}, "plain", "conv_stream_kernel<4, 2, false>"),
    ("stream_many_steps", (2, 64, 64, 40, 24, 2), {"USSEG_STREAM_MIN_STEPS": "1", "USSEG_STREAM_WGX": "8"}, "plain", "conv_stream_kernel<4, 4, false>"),
    ("big_128", (2, 32, 32, 256, 64, 1), {}, "plain", "conv_big_kernel<1, 2, 4>"),
    ("big_w8_forced", (2, 32, 32, 256, 64, 1), {"USSEG_BIG_W8": "2"}, "plain", "conv_big_kernel<1, 2, 8>"),
    ("big_accumulate", (2, 32, 32, 256, 64, 1), {}, "accumulate", "conv_big_kernel<1, 2, 4>"),
    ("halo", (2, 16, 16, 72, 136, 2), {}, "plain", "conv_halo_kernel<1>"),
    ("halo_accumulate", (3, 16, 16, 96, 40, 4), {}, "accumulate", "conv_halo_kernel<1>"),
    ("halo_view", (2, 32, 32, 48, 24, 4), {}, "view", "conv_halo_kernel<1>"),
    ("igemm_dma_view", (2, 10, 6, 16, 24, 2), {}, "view", "igemm_dma_kernel<1, 3>"),
    ("halo_res", (2, 16, 16, 72, 136, 2), {}, "res", "conv_halo_kernel<1>"),
    ("persist", (2, 256, 256, 16, 32, 1), {"USSEG_STREAM_MIN_STEPS": "1000000"}, "plain", "conv_halo_persist_kernel<1>"),
    ("persist_accumulate", (2, 256, 256, 16, 32, 1), {}, "accumulate", "conv_halo_persist_kernel<1>"),
    ("igemm_dma", (1, 12, 20, 32, 32, 1), {}, "plain", "igemm_dma_kernel<2, 3>"),
    ("igemm_dma_accumulate", (1, 24, 24, 128, 16, 4), {}, "accumulate", "igemm_dma_kernel<2, 3>"),
    ("igemm_1x1", (3, 7, 5, 40, 24, 1), {}, "plain", "igemm_kernel<2, 4>"),
]


@pytest.mark.parametrize("shape,env,epi,expect", [c[1:] for c in DGRAD], ids=[c[0] for c in DGRAD])
def test_dgrad_route(gen, monkeypatch, shape, env, epi, expect):
    B, H, W, Cin, Cout, dil = shape
    k = 1 if expect == "igemm_kernel<2, 4>" else 3
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    layer, w, b = make_conv(gen, Cin, Cout, k, dil)
    x = seam_data(gen, B, H, W, Cin)
    dy = seam_data(gen, B, H, W, Cout)
    layer.forward(to_dev(x)[1])
    bands = rows_checked(B, H)
    kw = {}
    base = None
    if epi in ("accumulate", "view"):
        base = bf(torch.randn(B, H, W, Cin, generator=gen, dtype=torch.float64))
        if epi == "view":
            dxbuf, dxd = to_dev(base, ld=layer.cin_p + 16, off=8, fill=1.0)
        else:
            dxbuf, dxd = to_dev(base)
        kw = dict(dx=dxd, accumulate_dx=True)
    if epi == "res":
        base = bf(torch.randn(B, H, W, Cin, generator=gen, dtype=torch.float64))
        kw = dict(dx_residual=to_dev(base)[1])
    dyd = to_dev(dy)[1]
    dx, _ = routed(lambda: layer.backward(dyd, skip_wgrad=True, skip_bias=True, **kw), expect)
    torch.cuda.synchronize()
    wd = w.flip(0, 1).transpose(2, 3)          # backward data of a stride-1 'SAME' conv: the flipped, transposed kernel
    ref = banded(lambda t: O.conv2d_same(t, wd, None, dil), dy, dil * (k // 2), bands)
    mag = banded(lambda t: O.conv2d_same(t.abs(), wd.abs(), None, dil), dy, dil * (k // 2), bands)
    if base is not None:
        ref, mag = ref + pick(base, bands), mag + pick(base.abs(), bands)
    assert_elementwise(pick(dx[..., :Cin], bands), ref, mag, U_BF16, 4.0, what=f"dgrad {expect}")
    if layer.cin_p > Cin and epi == "plain":
        assert dx[..., Cin:].abs().max().item() == 0, "pad channels"
    if epi == "view":
        assert (dxbuf[..., :8] == 1.0).all() and (dxbuf[..., 8 + layer.cin_p:] == 1.0).all(), "outside the dx view"


# ------------------------------------------------------------------------------------------------ multi-job launches
@pytest.mark.parametrize("shape,merge,expect", [
    ((1, 128, 128, 128, 16), "1", ["conv_stream_kernel<1, 4, false>"]),
    ((1, 128, 128, 128, 16), "0", ["conv_stream_kernel<1, 4, false>"] * 3),
    ((2, 64, 64, 64, 16), "1", ["conv_big_kernel<1, 2, 4>"]),
    ((2, 32, 32, 64, 16), "1", ["conv_halo_kernel<1>"]),
], ids=["stream_merged", "stream_unmerged", "big", "halo"])
def test_multi_job_route(gen, monkeypatch, shape, merge, expect):
    """Three dilated 3x3 branches (the decoder stage) in one conv2d_fwd_multi call: the kernel, the number of launches and every
    element of every branch."""
    from ultrasound_modeling_amd import ops
    B, H, W, Cin, q = shape
    monkeypatch.setenv("USSEG_STREAM_MERGE", merge)
    dil = (2, 4, 8)
    convs = [make_conv(gen, Cin, q, 3, d) for d in dil]
    x = seam_data(gen, B, H, W, Cin)
    xd = to_dev(x)[1]
    out = torch.full((B, H, W, 3 * q), 9.0, dtype=torch.bfloat16, device=DEV)
    _, got = routed(lambda: ops.conv2d_fwd_multi([(xd, c.wp_f, c.bias.data, 3, d, out[..., j * q:(j + 1) * q], ops.ACT_LRELU, ALPHA)
                                                  for j, ((c, _, _), d) in enumerate(zip(convs, dil))]), *expect)
    conv_launches = [g for g in got if g.startswith(("conv_", "igemm"))]
    assert len(conv_launches) == len(expect), got
    torch.cuda.synchronize()
    bands = rows_checked(B, H)
    for j, ((_, w, b), d) in enumerate(zip(convs, dil)):
        ref = act_ref(banded(lambda t: O.conv2d_same(t, w, b, d), x, d, bands), "lrelu")
        mag = banded(lambda t: O.conv2d_same(t.abs(), w.abs(), b.abs(), d), x, d, bands)
        assert_elementwise(pick(out[..., j * q:(j + 1) * q], bands), ref, mag, U_BF16, 4.0, what=f"branch {j}")


# ------------------------------------------------------------------------------------------------ weight gradients
# (id, (B, H, W, Cin, Cout, k, dil), expected kernels)
WGRAD = [
    ("wgrad_dma_tm1", (1, 12, 20, 32, 32, 3, 1), ["wgrad_dma_kernel<1, 3>"]),
    ("wgrad_dma_tm2", (1, 20, 20, 72, 136, 3, 8), ["wgrad_dma_kernel<2, 2>", "wgrad_finish_kernel"]),
    ("wgrad_dma_1x1", (3, 9, 7, 136, 200, 1, 1), ["wgrad_dma_kernel<2, 2>"]),
    ("wgrad_halo_1job", (2, 16, 16, 16, 32, 3, 1), ["wgrad_halo_kernel<2, 1, 1, true, 1, false>", "wgrad_finish_kernel"]),
    ("wgrad_halo_4x1x2", (5, 8, 8, 64, 24, 3, 1), ["wgrad_halo_kernel<4, 1, 2, true, 1, false>"]),
    ("wgrad_halo_4x1x1", (2, 256, 256, 64, 16, 3, 4), ["wgrad_halo_kernel<4, 1, 1, true, 1, false>", "wgrad_finish_kernel"]),
    ("wgrad_halo_8wave", (2, 16, 16, 72, 136, 3, 2), ["wgrad_halo_kernel<2, 2, 2, true, 2, false>", "wgrad_finish_kernel"]),
]


def _wgrad_refs(x, dy, w, k, dil):
    wr = w.clone().requires_grad_(True)
    (O.conv2d_same(x, wr, None, dil) * dy).sum().backward()
    wm = w.abs().clone().requires_grad_(True)
    (O.conv2d_same(x.abs(), wm, None, dil) * dy.abs()).sum().backward()
    return wr.grad, wm.grad


@pytest.mark.parametrize("shape,expect", [c[1:] for c in WGRAD], ids=[c[0] for c in WGRAD])
def test_wgrad_route(gen, shape, expect):
    from ultrasound_modeling_amd import ops
    B, H, W, Cin, Cout, k, dil = shape
    layer, w, b = make_conv(gen, Cin, Cout, k, dil)
    x = seam_data(gen, B, H, W, Cin)
    dy = seam_data(gen, B, H, W, Cout)
    layer.forward(to_dev(x)[1])
    dyd = to_dev(dy)[1]

    def run():
        layer.backward(dyd, need_dx=False)
        ops.defer_flush()
    routed(run, *expect)
    torch.cuda.synchronize()
    ref, mag = _wgrad_refs(x, dy, w, k, dil)
    assert_elementwise(layer.kernel.grad, ref, mag, U_F32, c_f32(B * H * W), what=f"wgrad {expect[0]}")
    assert_elementwise(layer.bias.grad, dy.sum((0, 1, 2)), dy.abs().sum((0, 1, 2)), U_F32, c_f32(B * H * W), what="bias grad")


@pytest.mark.parametrize("chans", [((32, 32), (16, 32), (1, 16)), ((24, 32), (32, 24), (8, 8))], ids=["three_jobs_a", "three_jobs_b"])
def test_wgrad_halo_multi_job_route(gen, chans):
    """Weight gradients of several convs with different channel counts in one wgrad_halo launch (conv2d_wgrad_multi)."""
    from ultrasound_modeling_amd import ops
    B, H, W = 2, 64, 64
    layers = [make_conv(gen, ci, co, 3, 1) for ci, co in chans]
    xs = [seam_data(gen, B, H, W, ci) for ci, _ in chans]
    dys = [seam_data(gen, B, H, W, co) for _, co in chans]
    jobs = []
    for (layer, _, _), x, dy in zip(layers, xs, dys):
        layer.forward(to_dev(x)[1])
        jobs.append(layer.wgrad_job(to_dev(dy)[1]))
    _, got = routed(lambda: ops.conv2d_wgrad_multi(jobs), "wgrad_halo_kernel<")
    assert sum(g.startswith("wgrad_halo_kernel") for g in got) == 1, got
    torch.cuda.synchronize()
    for (layer, w, _), x, dy in zip(layers, xs, dys):
        ref, mag = _wgrad_refs(x, dy, w, 3, 1)
        assert_elementwise(layer.kernel.grad, ref, mag, U_F32, c_f32(B * H * W), what="multi-job wgrad")


# ------------------------------------------------------------------------------------------------ transposed conv
# (id, (B, H, W, Cin, Cout, k), env, pass, expected kernel)
TCONV = [
    ("fwd_cls_nt1", (1, 8, 8, 72, 3, 3), {}, "fwd", "igemm_dma_kernel<1, 3>"),
    ("fwd_cls_nt2", (3, 9, 7, 136, 72, 4), {}, "fwd", "igemm_dma_kernel<2, 3>"),
    ("fwd_cls_f32", (1, 16, 16, 264, 136, 3), {}, "fwd_f32", "igemm_dma_kernel<2, 3>"),
    ("dgrad_cls", (1, 16, 16, 160, 64, 3), {}, "dgrad", "igemm_dma_kernel<2, 3>"),
    ("dgrad_cls_k4", (2, 3, 5, 24, 16, 4), {}, "dgrad", "igemm_dma_kernel<2, 3>"),
    ("wgrad_per_tap", (3, 9, 7, 136, 72, 4), {"USSEG_TCONV_HALO": "0"}, "wgrad", "wgrad_dma_kernel<2, 2>"),
    ("wgrad_masked_halo", (2, 16, 16, 160, 64, 4), {"USSEG_TCONV_HALO": "1"}, "wgrad", "wgrad_halo_kernel<"),
    ("wgrad_masked_halo_k3", (3, 32, 16, 24, 136, 3), {"USSEG_TCONV_HALO": "1"}, "wgrad", "wgrad_halo_kernel<"),
]


@pytest.mark.parametrize("shape,env,ps,expect", [c[1:] for c in TCONV], ids=[c[0] for c in TCONV])
def test_tconv_route(gen, monkeypatch, shape, env, ps, expect):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.flat import FlatParams
    from ultrasound_modeling_amd.layers import Conv2DTranspose
    B, H, W, Cin, Cout, k = shape
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    layer = Conv2DTranspose(Cin, Cout, k)
    w = bf(torch.randn(k, k, Cout, Cin, generator=gen, dtype=torch.float64) / math.sqrt(k * k * Cin))
    b = bf(torch.randn(Cout, generator=gen, dtype=torch.float64) * 0.5)
    layer.kernel.data.copy_(w)
    layer.bias.data.copy_(b)
    FlatParams(layer, DEV)
    x = seam_data(gen, B, H, W, Cin)
    xd = to_dev(x)[1]
    if ps.startswith("fwd"):
        f32 = ps == "fwd_f32"
        y, _ = routed(lambda: layer.forward(xd, out_f32=f32), expect)
        torch.cuda.synchronize()
        ref = O.conv2d_transpose_s2_same(x, w, b)
        mag = O.conv2d_transpose_s2_same(x.abs(), w.abs(), b.abs())
        u, c = (U_F32, c_f32(k * k * Cin)) if f32 else (U_BF16, 4.0)
        assert_elementwise(y[..., :Cout], ref, mag, u, c, what=f"tconv forward {expect}")
        if not f32 and layer.cout_p > Cout:
            assert y[..., Cout:].abs().max().item() == 0, "pad channels"
        return
    dy = seam_data(gen, B, 2 * H, 2 * W, Cout)
    layer.forward(xd)
    dyd = to_dev(dy)[1]
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xr, wr, b) * dy).sum().backward()
    xm, wm = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    (O.conv2d_transpose_s2_same(xm, wm, None) * dy.abs()).sum().backward()
    if ps == "dgrad":
        dx, _ = routed(lambda: ops.tconv2d_dgrad(dyd, layer.wp_d, k, ops.new_act(B, H, W, layer.cin_p, DEV)), expect)
        torch.cuda.synchronize()
        assert_elementwise(dx[..., :Cin], xr.grad, xm.grad, U_BF16, 4.0, what=f"tconv dgrad {expect}")
        return

    def run():
        layer.backward(dyd, need_dx=False)
        ops.defer_flush()
    routed(run, expect)
    torch.cuda.synchronize()
    assert_elementwise(layer.kernel.grad, wr.grad, wm.grad, U_F32, c_f32(4 * B * H * W), what=f"tconv wgrad {expect}")


# ------------------------------------------------------------------------------------------------ size guards
# igemm's LDS-DMA forms need 32-bit byte offsets (B*H*W*ldx*2 < 0x7fff0000) and pixel indices below 2^23 (fdivmod_px, signed
# 24-bit multiplies); past either limit the pass falls back to igemm_kernel (64-bit offsets, K step 64 for K >= 128).  One
# 1x1 conv just inside and one just outside each limit; the data is made on the device and checked over row bands.
# Cost on the MI355X: under 1 s per case (up to 4.3 GB of activations, fp64 reference over ~12 rows).
LIMITS = [
    ("px_inside", (1, 47, 178481, 64, 64), "igemm_dma_persist_kernel<1, 3>"),      # 2^23 - 1 pixels (1 GB: under the byte limit)
    ("px_outside", (1, 64, 131072, 64, 64), "igemm_kernel<1, 4>"),                # 2^23 pixels (K = 64: the K step stays 32)
    ("bytes_inside", (1, 25, 167767, 128, 256), "igemm_dma_persist_kernel<1, 3>"),  # 4194175 * 256 * 2 < 0x7fff0000
    ("bytes_outside", (1, 64, 65536, 128, 256), "igemm_kernel<1, 8>"),            # 4194304 * 256 * 2 > 0x7fff0000
]


@pytest.mark.parametrize("shape,expect", [c[1:] for c in LIMITS], ids=[c[0] for c in LIMITS])
def test_limit_edge_igemm(gen, shape, expect):
    from ultrasound_modeling_amd import ops
    B, H, W, Cin, ldx = shape
    Cout = 8
    layer, w, b = make_conv(gen, Cin, Cout, 1, 1)
    g = torch.Generator(device=DEV).manual_seed(99)
    xbuf = torch.randn(B, H, W, ldx, generator=g, device=DEV).to(torch.bfloat16)
    xd = xbuf[..., :Cin]
    xd[B - 1, H - 1, W - 1, Cin - 1] = 64.0
    y, _ = routed(lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=ALPHA), expect)
    torch.cuda.synchronize()
    del xbuf
    bands = rows_checked(B, H, force=True)
    xs = torch.cat([xd[bb:bb + 1, r:r + 1].double().cpu() for bb, rows in bands for r in rows])
    ref = act_ref(O.conv2d_same(xs, w, b, 1), "lrelu")[:, 0]
    mag = O.conv2d_same(xs.abs(), w.abs(), b.abs(), 1)[:, 0]
    assert_elementwise(pick(y[..., :Cout], bands), ref, mag, U_BF16, 4.0, what=f"limit {expect}")


# The conv_big / conv_stream planners (big_fill_job) refuse launches of B*H*W*ldx >= 2^30 elements or B*H*W >= 2^23 pixels; the
# pass then falls to conv_halo (64-bit pixel offsets), here its persistent form.  3x3 convs of 8 -> 8 channels on 256x256 images:
# one image short of each limit, and the limit itself.  The third guard there, npatches < 2^20, cannot bind first: every tiling it
# accepts has >= 16 pixels per patch, so npatches <= B*H*W / 16 < 2^19 whenever the pixel guard holds (the same holds for
# wgrad_halo's npatches guard).  Checked over row bands of the first and last image.  Cost: about 1 s per case.
CONV_LIMITS = [
    ("px_inside", 127, 8, "conv_stream_kernel<1, 4, false>"),        # 127 * 2^16 pixels
    ("px_outside", 128, 8, "conv_halo_persist_kernel<1>"),           # 2^23 pixels
    ("bytes_inside", 63, 256, "conv_stream_kernel<1, 4, false>"),    # 63 * 2^16 * 256 elements < 2^30
    ("bytes_outside", 64, 256, "conv_halo_persist_kernel<1>"),       # 2^30 elements
]


def dev_data(B, H, W, C, ld, seed):
    """Device bf16 [B,H,W,C] view (channels 0..C of a zeroed buffer with `ld` channels) of seeded normal data, last element 64."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.zeros(B, H, W, ld, dtype=torch.bfloat16, device=DEV)
    for b in range(0, B, 16):
        buf[b:b + 16, ..., :C] = torch.randn(min(16, B - b), H, W, C, generator=g, device=DEV).to(torch.bfloat16)
    v = buf[..., :C]
    v[B - 1, H - 1, W - 1, C - 1] = 64.0
    return buf, v


@pytest.mark.parametrize("B,ld,expect", [c[1:] for c in CONV_LIMITS], ids=[c[0] for c in CONV_LIMITS])
def test_limit_edge_conv_planner(gen, B, ld, expect):
    from ultrasound_modeling_amd import ops
    H = W = 256
    layer, w, b = make_conv(gen, 8, 8, 3, 1)
    buf, xd = dev_data(B, H, W, 8, ld, 7)
    y, _ = routed(lambda: layer.forward(xd, act=ops.ACT_LRELU, alpha=ALPHA), expect)
    torch.cuda.synchronize()
    bands = rows_checked(B, H, force=True)
    refs, mags, ys = [], [], []
    for bb, rows in bands:
        for r in rows:
            lo, hi = max(0, r - 1), min(H, r + 2)
            xs = xd[bb:bb + 1, lo:hi].double().cpu()
            refs.append(act_ref(O.conv2d_same(xs, w, b, 1)[:, r - lo], "lrelu"))
            mags.append(O.conv2d_same(xs.abs(), w.abs(), b.abs(), 1)[:, r - lo])
            ys.append(y[bb:bb + 1, r, :, :8])
    assert_elementwise(torch.cat(ys), torch.cat(refs), torch.cat(mags), U_BF16, 4.0, what=f"limit {expect}")


# Weight-gradient guards.  wgrad_halo (3x3) needs B*H*W < 2^23 and B*H*W*ldx < 2^31 (32-bit element offsets); past them the pass
# goes to launch_wgrad, whose LDS-DMA kernel needs B*H*W*ldx*2 < 0x7fff0000 and H*W < 2^23 - and past those it runs wgrad_kernel
# (64-bit offsets).  The fp64 reference of these full-tensor reductions is taken on the device (torch fp64 contractions of the
# same bf16 data): there are no row bands of a weight gradient.  Cost: about 1 s per case.
WGRAD_LIMITS = [
    # (id, (B, H, W, ld), k, expected)
    ("halo_px_inside", (127, 256, 256, 8), 3, "wgrad_halo_kernel<"),
    ("halo_px_outside", (128, 256, 256, 8), 3, "wgrad_dma_kernel<1, 3>"),
    ("halo_offsets_inside", (63, 256, 256, 512), 3, "wgrad_halo_kernel<"),     # 63 * 2^16 * 512 < 2^31
    ("halo_offsets_outside", (64, 256, 256, 512), 3, "wgrad_kernel"),          # 2^31 elements: also past the LDS-DMA byte limit
    ("dma_bytes_inside", (1, 25, 167767, 256), 1, "wgrad_dma_kernel<1, 3>"),   # 4194175 * 256 * 2 < 0x7fff0000
    ("dma_bytes_outside", (1, 64, 65536, 256), 1, "wgrad_kernel"),
    ("dma_px_inside", (1, 47, 178481, 8), 1, "wgrad_dma_kernel<1, 3>"),        # 2^23 - 1 pixels in one image
    ("dma_px_outside", (1, 64, 131072, 8), 1, "wgrad_kernel"),                 # 2^23
]


def wgrad_ref_dev(x, dy, k):
    """fp64 dw[kh, kw, ci, co] of a stride-1 'SAME' conv (dilation 1), computed on the device."""
    B, H, W, C = x.shape
    p = k // 2
    xp = torch.zeros(B, H + 2 * p, W + 2 * p, C, dtype=torch.float64, device=x.device)
    xp[:, p:p + H, p:p + W] = x
    d = dy.reshape(-1, dy.shape[-1])
    return torch.stack([torch.stack([xp[:, i:i + H, j:j + W].reshape(-1, C).T @ d for j in range(k)]) for i in range(k)])


@pytest.mark.parametrize("shape,k,expect", [c[1:] for c in WGRAD_LIMITS], ids=[c[0] for c in WGRAD_LIMITS])
def test_limit_edge_wgrad(shape, k, expect):
    from ultrasound_modeling_amd import ops
    B, H, W, ld = shape
    C = 8
    xbuf, xd = dev_data(B, H, W, C, ld, 11)
    dybuf, dyd = dev_data(B, H, W, C, C, 12)
    dw = torch.zeros(k, k, C, C, dtype=torch.float32, device=DEV)
    routed(lambda: ops.conv2d_wgrad(xd, dyd, k, 1, dw), expect)
    torch.cuda.synchronize()
    x64, dy64 = xd.double(), dyd.double()
    del xbuf
    ref = wgrad_ref_dev(x64, dy64, k)
    mag = wgrad_ref_dev(x64.abs_(), dy64.abs_(), k)
    assert_elementwise(dw, ref, mag, U_F32, c_f32(B * H * W), what=f"wgrad limit {expect}")


# Batched GEMMs (the nb2 forms of igemm and of the weight-gradient kernels, used by the attention blocks): the LDS-DMA kernels
# when the K loop is long enough and the batch bases are 16-byte aligned; igemm_kernel for K < 32; wgrad_kernel past K = 2^23.
@pytest.mark.parametrize("M,N,K,expect", [(200, 40, 72, "igemm_dma_kernel<"), (200, 40, 24, "igemm_kernel<")], ids=["dma", "short_k"])
def test_batched_gemm_nt_route(M, N, K, expect):
    from ultrasound_modeling_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(2, 3, M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = torch.randn(2, 3, N, K, generator=g, device=DEV).to(torch.bfloat16)
    y = torch.full((2, 3, M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    routed(lambda: ops.gemm_nt_batched(x, w, y, M, N, K, K, K, N, 2, 3, (3 * M * K, M * K), (3 * N * K, N * K), (3 * M * N, M * N)), expect)
    torch.cuda.synchronize()
    ref = torch.einsum("abmk,abnk->abmn", x.double(), w.double())
    mag = torch.einsum("abmk,abnk->abmn", x.double().abs(), w.double().abs())
    assert_elementwise(y, ref, mag, U_BF16, 4.0, what=f"gemm_nt_batched {expect}")


@pytest.mark.parametrize("M,N,K,expect", [(40, 72, 1000, "wgrad_dma_kernel<1, 3>"), (8, 8, 1 << 23, "wgrad_kernel")], ids=["dma", "k_limit"])
def test_batched_gemm_tn_route(M, N, K, expect):
    from ultrasound_modeling_amd import ops
    g = torch.Generator(device=DEV).manual_seed(6)
    a = torch.randn(1, 2, K, M, generator=g, device=DEV).to(torch.bfloat16)
    b = torch.randn(1, 2, K, N, generator=g, device=DEV).to(torch.bfloat16)
    out = torch.zeros(1, 2, M, N, dtype=torch.float32, device=DEV)
    routed(lambda: ops.gemm_tn_batched(a, b, out, M, N, K, M, N, 1, 2, (2 * K * M, K * M), (2 * K * N, K * N), (2 * M * N, M * N)), expect)
    torch.cuda.synchronize()
    ref = torch.einsum("abkm,abkn->abmn", a.double(), b.double())
    mag = torch.einsum("abkm,abkn->abmn", a.double().abs(), b.double().abs())
    assert_elementwise(out, ref, mag, U_F32, c_f32(K), what=f"gemm_tn_batched {expect}")
