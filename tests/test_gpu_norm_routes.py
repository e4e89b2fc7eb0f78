"""Norm / split-attention route matrix (GPU): every route of the LayerNorm / BatchNorm + activation kernels, their split-attention
forms, the lane-per-pixel LayerNorm backward tiles and the split-attention pool / MLP / re-weighting, with a per-element bound.

Each case first asserts WHICH kernels it launched (route_probe.routed), then checks every output element against an fp64
restatement built from oracle/usseg_oracle.py (layer_norm, batch_norm, the activations, softmax_lastaxis) on the same bf16-exact
inputs, pad channels for exact zeros, and - for channel-slice views - that the elements outside the view (NaN-filled) are untouched.
Inputs follow route_probe.seam_data: one rare large element and a last image that is non-zero only near the 16-row seams and at
the tail.  Routes are driven by shapes only: USSEG_LN_TILE, USSEG_LN_TILE_MIN, USSEG_LN_PAIR and USSEG_LOSS_PPT are read once per
process and are never set here.

Bounds (|y - ref| <= c*u*mag + tiny for every element; mag = the same operation on absolute values):
  * bf16 outputs: u = 2^-8, c = 4.
    - LN / BN forward: mag = |gamma*xhat| + |beta| (times the mask value where there is one).
    - backward dx, with g = act'(pre)*dy: LayerNorm and batch-statistics BN: mag = rstd*(|gamma*g| + mean|gamma*g| +
      |xhat|*mean|gamma*g*xhat|), the means over the group (LN) or over the M pixels (BN); affine BN: mag = rstd*|gamma*g|.
      FUSE forms: g is built from |dout|*|mult*s| + |dg|.  RES: + |dres|, c = 8 (two roundings).
    - split-attention output: mag = mult*sum_r |y_r|*mag(s); its dy: mag = mult*mag(s)*|dout| + mag(dg).  The MLP is restated
      on absolute values (every matrix as |W|, LN' as above, softmax' -> mag(s)*(|ds| + sum mag(s)*|ds|)); its forward values are
      fp32 results of its own, so their mags carry their sensitivity: xhat -> rstd*(mag(h1) + mean mag(h1)), a -> |gamma|*mag(xhat)
      + |beta|, s -> s*(1 + mag(z) + sum s*mag(z)).
  * fp32 sums (dgamma, dbeta, dbias, gap rows, batch mean / variance, moving statistics, MLP parameter gradients): u = 2^-20,
    c = 4 + sqrt(K)/8 with K the number of summed pixels, mag = the sum of |terms| (the batch variance: mean((x - mu)^2)).
  * Kink rule (LeakyReLU / ReLU): an element whose fp64 pre-activation lies within 2^-12*mag of 0 may take the other slope in
    fp32.  Those elements are left out of the dx check (counted, at most 0.1 % of the checked elements), and the slope they could
    have taken is added to the bound of what they feed: (1 - slope)*|gamma*dy| through the group means of the other elements of
    their group (LN) or channel (BN), and into dgamma / dbeta / dbias; in the split-attention MLP, into the mags of everything
    downstream of that pre-activation.
Each checked output prints its worst ratio err / bound (run with -s to read them).

Routes, and the kernels their cases assert:
  * norm_act_kernel<*, 0, NG> LayerNorm (NG = 1 for G = 1, 3 for G = 2 and 3, 4 for G = 4), lanes per pixel 1..64, activations
    none / LReLU / ReLU / ELU, strided views; past both grid caps (test_layernorm_streaming).
  * norm_act_kernel<*, 1, 1> BN inference with the dropout mask operand (test_batchnorm_inference_mask).
  * norm_act_kernel<true, 2, 1> backward from the activated output, gamma of both signs (test_batchnorm_mode2).
  * norm_act_kernel<true, 0, 1, false, false, true> (test_layernorm_backward_res).
  * norm_act_kernel<false, *, *, true> (norm_act_fwd_gap) with nb > 1 gap rows, norm_act_kernel<true, *, *, true> (norm_act_bwd_sa)
    including the HW % 64 != 0 fallback at M >= 32768 (test_norm_fused_split_attention).
  * ln_bwd_tile_kernel<CP, CG, NG, false>: the 12 table geometries, ragged M, and the streaming kernel just below the size floor,
    off the table, with a mask and for ELU (test_ln_tile); ln_bwd_tile_kernel<..., true>: the 8 fused geometries
    (test_ln_tile_fused); ln_bwd_pair_kernel: both instantiations (test_ln_pair).
  * reduce_finish_batched_kernel inside ops.overlap_region (test_norm_deferred_finish).
  * bn_act_pool_kernel<false> + norm_act_kernel<true, 1, 1, false, true> with power-of-two and divided pixel decodes (test_bn_act_pool).
  * colsum_kernel<2> -> bn_batch_finalize_kernel -> mode 1 -> bn_train_bwd_fix_kernel, |mean| up to 100 std (test_batchnorm_batch_statistics).
  * sa_reduce_kernel (gx = 1, gx > 1, gx capped at 64 and at 1024 / B), sa_mlp_kernel<false / true>, sa_apply_kernel<false / true>
    (test_split_attention); the guard limits Cg = 128, Hd = 64, R = 4 run, Cg = 129 / Hd = 65 / R = 5 are refused before any launch.
Routes no shape reaches: none of this family.  sa_reduce_kernel's grid width is not part of its name: the cases choose HW, B and Cy
so that gx = 1, gx > 1 and both caps hold by the launcher's arithmetic (stated beside each case).
"""
import math

import pytest
import torch

import usseg_oracle as O
from route_probe import (ACTS, EPS, U_BF16, U_F32, act_f, bf, c_f32, check, check_norm_bwd, kname, nan_view, ng_of, no_launch, norm_ref, outside_untouched,
                         routed, sa_reference, seam_data, small_deferral, to_dev)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def vec(gen, n, base=1.0, sc=0.3, neg=False):
    v = (base + sc * torch.randn(n, generator=gen, dtype=torch.float64)).float().double()
    if neg:
        v[::3] = -v[::3]
    return v


def padded(v, cp):
    return torch.cat([v.float(), torch.zeros(cp - v.numel())]).to(DEV)


# ------------------------------------------------------------------------------------------------ streaming LayerNorm
# (id, (B, H, W), C, G, act, view): Cphys = roundup(C, 8) sets the lanes per pixel (Cphys/8 chunks rounded up to a power of two)
LN_STREAM = [
    ("lpp1", (2, 9, 13), 5, 1, "lrelu", False),
    ("lpp2", (2, 9, 13), 13, 1, "relu", True),
    ("lpp4_idle_lane", (3, 7, 11), 21, 1, "elu", False),
    ("lpp8", (2, 9, 13), 37, 1, "none", True),
    ("lpp16", (2, 9, 13), 70, 1, "lrelu", False),
    ("lpp32", (2, 5, 13), 131, 1, "relu", False),
    ("lpp64_264", (2, 5, 13), 260, 1, "elu", True),
    ("lpp64_512", (2, 5, 7), 509, 1, "lrelu", False),
    ("g2", (2, 9, 13), 26, 2, "lrelu", False),          # G = 2 runs the NG = 3 kernel with one group unused
    ("g2_view", (2, 6, 7), 50, 2, "elu", True),
    ("g3", (2, 9, 13), 33, 3, "relu", False),
    ("g3_wide", (1, 5, 9), 255, 3, "lrelu", True),
    ("g4", (2, 9, 13), 36, 4, "none", False),
    ("g4_view", (2, 6, 7), 60, 4, "lrelu", True),
    # grid caps at Cphys 512 (4 pixels per workgroup trip): backward 1024 * 2 * 4 = 8192, forward 2048 * 4 * 4 = 32768 pixels
    ("caps_bwd_relu", (2, 72, 72), 509, 1, "relu", False),
    ("caps_fwd_none", (1, 136, 256), 512, 1, "none", False),
    ("caps_g3_elu", (2, 72, 72), 501, 3, "elu", False),
]


@pytest.fixture(scope="module")
def gen():
    return torch.Generator().manual_seed(2468)


def run_norm_case(gen, what, shape, C, G, act, mode=0, view=False, mask=False, fwd_kernel=None, bwd_kernels=(), neg_gamma=False):
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    M, cp = B * H * W, (C + 7) // 8 * 8
    A, alpha = ACTS[act]
    x = seam_data(gen, B, H, W, C)
    dy = seam_data(gen, B, H, W, C)
    gamma, beta = vec(gen, C, neg=neg_gamma), vec(gen, C, 0.0, 0.2)
    mean = var = mk = mkd = None
    if mode == 1:
        mean, var = vec(gen, C, 0.0, 0.3), (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float().double()
    if mask:
        mk = bf((torch.rand(B, H, W, C, generator=gen) < 0.7).double() * 2.0)
        mkbuf, mkd = to_dev(mk, ld=cp + 8 if view else None, off=8 if view else 0, fill=NAN)
    if view:
        xbuf, xd = to_dev(x, ld=cp + 16, off=8, fill=NAN)
        dybuf, dyd = to_dev(dy, ld=cp + 32, off=24, fill=NAN)
        ybuf, yd = nan_view(B, H, W, cp, cp + 24, 16)
        dxbuf, dxd = nan_view(B, H, W, cp, cp + 8, 8)
    else:
        xd, dyd = to_dev(x)[1], to_dev(dy)[1]
        yd, dxd = torch.full_like(xd, NAN), torch.full_like(xd, NAN)
    dvec = lambda v: None if v is None else padded(v, cp)
    kw = dict(mean=dvec(mean), var=dvec(var))
    y, _ = routed(lambda: ops.norm_act_fwd(xd, C, dvec(gamma), dvec(beta), yd, mode, G, EPS, A, alpha, mask=mkd, **kw), fwd_kernel)
    dg, db, dbias = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    dx, _ = routed(lambda: ops.norm_act_bwd(xd, dyd, C, dvec(gamma), dvec(beta), dxd, dg, db, mode, G, EPS, A, alpha, dbias=dbias, mask=mkd, **kw),
                   *bwd_kernels)
    torch.cuda.synchronize()
    dev = lambda t: None if t is None else t.to(DEV)
    ref = norm_ref(x.reshape(M, C).to(DEV), dev(gamma), dev(beta), act, G, mode, dev(mean), dev(var),
                   None if mk is None else mk.reshape(M, C).to(DEV), dy.reshape(M, C).to(DEV))
    check(f"{what} y", y[..., :C].reshape(M, C), ref["y"], ref["ymag"], U_BF16, 4.0)
    check_norm_bwd(what, M, C, ref, dx[..., :C].reshape(M, C), dg, db, dbias)
    if cp > C:
        assert y[..., C:].abs().max().item() == 0 and dx[..., C:].abs().max().item() == 0, "pad channels"
    if view:
        outside_untouched(ybuf, 16, cp, "y")
        outside_untouched(dxbuf, 8, cp, "dx")
    return ref


@pytest.mark.parametrize("shape,C,G,act,view", [c[1:] for c in LN_STREAM], ids=[c[0] for c in LN_STREAM])
def test_layernorm_streaming(gen, shape, C, G, act, view):
    ng = ng_of(G)
    run_norm_case(gen, f"LN {shape} C{C} G{G} {act}", shape, C, G, act, view=view,
                  fwd_kernel=kname(False, 0, ng), bwd_kernels=(kname(True, 0, ng), "reduce_finish_kernel"))


@pytest.mark.parametrize("act", ["none", "lrelu", "relu", "elu"])
@pytest.mark.parametrize("C,view", [(24, False), (45, True)], ids=["c24", "c45_view"])
def test_batchnorm_inference_mask(gen, act, C, view):
    """Affine BN (moving statistics) + activation with the dropout-mask operand on the forward and the backward."""
    run_norm_case(gen, f"BN mask C{C} {act}", (2, 9, 13), C, 1, act, mode=1, view=view, mask=True,
                  fwd_kernel=kname(False, 1, 1), bwd_kernels=(kname(True, 1, 1), "reduce_finish_kernel"))


@pytest.mark.parametrize("act", ["none", "lrelu", "relu"])
@pytest.mark.parametrize("neg", [False, True], ids=["pos_gamma", "neg_gamma"])
def test_batchnorm_mode2(gen, act, neg):
    """Backward from the ACTIVATED output y of a conv-epilogue-folded BN: the kernel recovers xhat = (act^-1(y) - beta)/gamma and
    takes the slope from the sign of y.  The reference is that maths in fp64 on the bf16 y the kernel reads."""
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 11, 9, 29
    M, cp = B * H * W, 32
    A, alpha = ACTS[act]
    x = seam_data(gen, B, H, W, C)
    gamma, beta = vec(gen, C, neg=neg), vec(gen, C, 0.0, 0.2)
    mean, var = vec(gen, C, 0.0, 0.3), (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float().double()
    y = bf(act_f(O.batch_norm(x, gamma, beta, mean, var, training=False), act))
    dy = seam_data(gen, B, H, W, C)
    ybuf, yd = to_dev(y, ld=cp + 8, off=8, fill=NAN)
    dyd = to_dev(dy)[1]
    dg, db, dbias = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    dxbuf, dxd = nan_view(B, H, W, cp, cp + 16, 16)
    dx, _ = routed(lambda: ops.norm_act_bwd(yd, dyd, C, padded(gamma, cp), padded(beta, cp), dxd, dg, db, 2, 1, EPS, A, alpha,
                                            padded(mean, cp), padded(var, cp), dbias=dbias), kname(True, 2, 1), "reduce_finish_kernel")
    torch.cuda.synchronize()
    yv, dyv = y.reshape(M, C), dy.reshape(M, C)
    neg_slope = {"lrelu": alpha, "relu": 0.0, "none": 1.0}[act]
    pre = torch.where(yv >= 0, yv, yv / alpha) if act == "lrelu" else yv
    xh = (pre - beta) / gamma
    rstd = (var + EPS).rsqrt()
    dh = dyv * torch.where(yv > 0, 1.0, neg_slope)
    check("mode2 dx", dx[..., :C].reshape(M, C), dh * gamma * rstd, (dh * gamma * rstd).abs(), U_BF16, 4.0)
    check("mode2 dgamma", dg[:C], (dh * xh).sum(0), (dh * xh).abs().sum(0), U_F32, c_f32(M))
    check("mode2 dbeta", db[:C], dh.sum(0), dh.abs().sum(0), U_F32, c_f32(M))
    check("mode2 dbias", dbias[:C], (dh * gamma * rstd).sum(0), (dh * gamma * rstd).abs().sum(0), U_F32, c_f32(M))
    assert dx[..., C:].abs().max().item() == 0, "pad channels"
    outside_untouched(dxbuf, 16, cp, "dx")


@pytest.mark.parametrize("C,shape", [(8, (2, 9, 13)), (40, (3, 7, 5)), (512, (2, 72, 72))], ids=["c8", "c40", "c512_caps"])
def test_layernorm_backward_res(gen, C, shape):
    """dx = bf16(bf16(LN'(dy)) + dres) with dres and dx as strided views; dbias = the column sums of the STORED dx."""
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    M = B * H * W
    x, dy, dres = (seam_data(gen, B, H, W, C) for _ in range(3))
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    xd, dyd = to_dev(x)[1], to_dev(dy)[1]
    rbuf, rd = to_dev(dres, ld=C + 16, off=16, fill=NAN)
    dxbuf, dxd = nan_view(B, H, W, C, C + 8, 8)
    dg, db, dbias = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx, _ = routed(lambda: ops.norm_act_bwd_res(xd, dyd, C, gamma.float().to(DEV), beta.float().to(DEV), rd, dxd, dg, db, EPS, dbias),
                   kname(True, 0, 1, res=True), "reduce_finish_kernel")
    torch.cuda.synchronize()
    ref = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), "none", dy=dy.reshape(M, C).to(DEV))
    r = dres.reshape(M, C).to(DEV)
    got = dx.reshape(M, C).double()
    check(f"res C{C} dx", got, ref["dx"] + r, ref["dxmag"] + r.abs(), U_BF16, 8.0)
    check(f"res C{C} dgamma", dg, ref["dgamma"], ref["dgmag"], U_F32, c_f32(M))
    check(f"res C{C} dbeta", db, ref["dbeta"], ref["dbmag"], U_F32, c_f32(M))
    check(f"res C{C} dbias", dbias, got.sum(0), got.abs().sum(0), U_F32, c_f32(M))
    outside_untouched(dxbuf, 8, C, "dx")
    outside_untouched(rbuf, 16, C, "dres")


# ------------------------------------------------------------------------------------------------ split-attention norm forms
def sa_vectors(gen, B, C, mult):
    s = torch.rand(B, C, generator=gen, dtype=torch.float64).float().double()
    dgv = (0.05 * torch.randn(B, C, generator=gen, dtype=torch.float64)).float().double()
    return s, dgv


def run_fused_bwd(gen, what, shape, C, G, act, expect, mode=0):
    """norm_act_bwd_sa: the incoming gradient is mult*s[b][c]*dout + dg[b][c], formed in registers."""
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    M, cp = B * H * W, (C + 7) // 8 * 8
    A, alpha = ACTS[act]
    mult = 3.0
    x, dout = seam_data(gen, B, H, W, C), seam_data(gen, B, H, W, C)
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    mean = var = None
    if mode == 1:
        mean, var = vec(gen, C, 0.0, 0.3), (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float().double()
    s, dgv = sa_vectors(gen, B, C, mult)
    xd, dod = to_dev(x)[1], to_dev(dout)[1]
    dg, db, dbias = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    dxbuf, dxd = nan_view(B, H, W, cp, cp + 8, 8)
    dvec = lambda v: None if v is None else padded(v, cp)
    dx, _ = routed(lambda: ops.norm_act_bwd_sa(xd, dod, C, padded(gamma, cp), padded(beta, cp), dxd, dg, db, mode, G, EPS, A, alpha,
                                               s.float().to(DEV), dgv.float().to(DEV), mult, dvec(mean), dvec(var), dbias=dbias), *expect)
    torch.cuda.synchronize()
    HW = H * W
    se = s.to(DEV).repeat_interleave(HW, 0)
    ge = dgv.to(DEV).repeat_interleave(HW, 0)
    do = dout.reshape(M, C).to(DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    ref = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), act, G, mode, dev(mean), dev(var), dy=mult * se * do + ge)
    # mags from |dout|*|mult*s| + |dg|: recompute with that gradient (the reference dx above keeps the signed one)
    mref = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), act, G, mode, dev(mean), dev(var), dy=mult * se * do.abs() + ge.abs())
    for k in ("dxmag", "dxext", "kink", "dgmag", "dbmag", "dgext", "dbext"):
        ref[k] = mref[k] if k != "kink" else ref["kink"] | mref["kink"]
    check_norm_bwd(what, M, C, ref, dx[..., :C].reshape(M, C), dg, db, dbias)
    if cp > C:
        assert dx[..., C:].abs().max().item() == 0, "pad channels"
    outside_untouched(dxbuf, 8, cp, "dx")


@pytest.mark.parametrize("shape,C,G,act,mode", [
    ((2, 16, 24), 30, 3, "lrelu", 0),
    ((3, 8, 40), 63, 3, "elu", 0),
    ((2, 16, 16), 64, 1, "relu", 1),
    ((1, 32, 64), 255, 3, "lrelu", 0),
], ids=["c30_g3", "c63_g3_elu", "bn_c64", "c255_g3"])
def test_norm_fused_split_attention(gen, shape, C, G, act, mode):
    """norm_act_fwd_gap (nb > 1 partial rows of the pool, each checked against an fp64 sum of the kernel's own bf16 y over that
    row's pixels) and the streaming norm_act_bwd_sa."""
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    M, cp, HW = B * H * W, (C + 7) // 8 * 8, H * W
    A, alpha = ACTS[act]
    ng = ng_of(G) if mode == 0 else 1
    x = seam_data(gen, B, H, W, C)
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    mean = var = None
    if mode == 1:
        mean, var = vec(gen, C, 0.0, 0.3), (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float().double()
    dvec = lambda v: None if v is None else padded(v, cp)
    xd = to_dev(x)[1]
    (y, (rows, nb, _)), _ = routed(lambda: ops.norm_act_fwd_gap(xd, C, padded(gamma, cp), padded(beta, cp), torch.full_like(xd, NAN), mode, G, EPS,
                                                                A, alpha, dvec(mean), dvec(var)), kname(False, mode, ng, fuse=True))
    torch.cuda.synchronize()
    assert nb > 1
    dev = lambda t: None if t is None else t.to(DEV)
    ref = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), act, G, mode, dev(mean), dev(var))
    check(f"gap {C} y", y[..., :C].reshape(M, C), ref["y"], ref["ymag"], U_BF16, 4.0)
    ppb = 4 * (64 // (1 << max(0, (cp // 8 - 1).bit_length())))
    yv = y.reshape(B, HW, cp).double()
    row_of = (torch.arange(HW, device=DEV) // ppb) % nb
    want = torch.stack([torch.stack([yv[b][row_of == r].sum(0) for r in range(nb)]) for b in range(B)])
    mag = torch.stack([torch.stack([yv[b][row_of == r].abs().sum(0) for r in range(nb)]) for b in range(B)])
    check(f"gap {C} rows", rows, want, mag, U_F32, c_f32(HW))
    run_fused_bwd(gen, f"bwd_sa C{C}", shape, C, G, act, (kname(True, mode, ng, fuse=True), "reduce_finish_kernel"), mode=mode)


def test_norm_fused_fallback_ragged_images(gen):
    """M >= 32768 with HW % 64 != 0: the fused tile cannot keep a tile inside one image, the streaming FUSE kernel runs."""
    run_fused_bwd(gen, "bwd_sa fallback", (2, 130, 127), 30, 3, "lrelu", (kname(True, 0, 3, fuse=True), "reduce_finish_kernel"))


# ------------------------------------------------------------------------------------------------ LayerNorm backward tiles
TILE_GEOMS = [(2, 3, 3), (3, 7, 3), (6, 14, 3), (11, 28, 3), (4, 10, 3), (8, 21, 3), (16, 42, 3), (32, 85, 3),
              (8, 64, 1), (16, 128, 1), (32, 256, 1), (64, 512, 1)]


def tile_case(gen, what, shape, CP, CG, NG, act="lrelu", mask=False, expect=None):
    C = CG * NG
    assert (C + 7) // 8 == CP
    run_norm_case(gen, what, shape, C, NG, act, mask=mask, fwd_kernel=kname(False, 0, ng_of(NG)), bwd_kernels=expect)


@pytest.mark.parametrize("geom", TILE_GEOMS, ids=[f"cp{g[0]}_cg{g[1]}_ng{g[2]}" for g in TILE_GEOMS])
def test_ln_tile(gen, geom):
    CP, CG, NG = geom
    tile_case(gen, f"tile {geom}", (2, 128, 128), CP, CG, NG, expect=(f"ln_bwd_tile_kernel<{CP}, {CG}, {NG}, false>", "reduce_finish_kernel"))


@pytest.mark.parametrize("geom", [(2, 3, 3), (16, 128, 1)], ids=["cp2", "cp16"])
def test_ln_tile_ragged(gen, geom):
    """M = 129 * 257 = 33153 (M % 64 = 1): the last tile holds one pixel."""
    CP, CG, NG = geom
    tile_case(gen, f"tile ragged {geom}", (1, 129, 257), CP, CG, NG, expect=(f"ln_bwd_tile_kernel<{CP}, {CG}, {NG}, false>",))


@pytest.mark.parametrize("shape,geom,act,mask,ng", [
    ((1, 181, 181), (2, 3, 3), "lrelu", False, 3),      # M = 32761: below the tile floor
    ((2, 128, 128), (4, 32, 1), "lrelu", False, 1),     # Cphys 32 with one group of 32: not in the table
    ((2, 128, 128), (8, 64, 1), "lrelu", True, 1),      # a dropout mask
    ((2, 128, 128), (8, 64, 1), "elu", False, 1),       # not LeakyReLU
], ids=["below_floor", "off_table", "mask", "elu"])
def test_ln_tile_streaming_fallback(gen, shape, geom, act, mask, ng):
    CP, CG, NG = geom
    tile_case(gen, f"tile fallback {geom} {act}", shape, CP, CG, NG, act=act, mask=mask, expect=(kname(True, 0, ng), "reduce_finish_kernel"))


@pytest.mark.parametrize("geom", TILE_GEOMS[:8], ids=[f"cp{g[0]}_cg{g[1]}" for g in TILE_GEOMS[:8]])
def test_ln_tile_fused(gen, geom):
    CP, CG, NG = geom
    run_fused_bwd(gen, f"tile fused {geom}", (2, 128, 128), CG * NG, NG, "lrelu", (f"ln_bwd_tile_kernel<{CP}, {CG}, {NG}, true>", "reduce_finish_kernel"))


def ln_pair_case(gen, ca, cb):
    """The shortcut norm (A) and conv2_bn with the re-weighting's backward (B) of one ln_bwd_pair_kernel launch: (outputs() -> fresh
    (dxa, dxb, [dgamma, dbeta, dbias of A, then of B]), launch(dxa, dxb, outs), check(dxa, dxb, outs) - every element bounded)."""
    from ultrasound_modeling_amd import ops
    B, H, W = 2, 128, 128
    M, cpb, HW = B * H * W, (cb + 7) // 8 * 8, H * W
    alpha, mult = ACTS["lrelu"][1], 3.0
    xa, dya, xb, dob = (seam_data(gen, B, H, W, c) for c in (ca, ca, cb, cb))
    ga, ba, gb, bb = vec(gen, ca, neg=True), vec(gen, ca, 0.0, 0.2), vec(gen, cb, neg=True), vec(gen, cb, 0.0, 0.2)
    s, dgv = sa_vectors(gen, B, cb, mult)

    def outputs():
        return (torch.full((B, H, W, ca), NAN, dtype=torch.bfloat16, device=DEV), torch.full((B, H, W, cpb), NAN, dtype=torch.bfloat16, device=DEV),
                [torch.zeros(c, device=DEV) for c in (ca, ca, ca, cpb, cpb, cpb)])

    def launch(dxa, dxb, outs):
        return ops.norm_act_bwd_pair(to_dev(xa)[1], to_dev(dya)[1], ca, ga.float().to(DEV), ba.float().to(DEV), dxa, *outs[:3], to_dev(xb)[1],
                                     to_dev(dob)[1], cb, 3, padded(gb, cpb), padded(bb, cpb), dxb, *outs[3:], s.float().to(DEV), dgv.float().to(DEV),
                                     mult, EPS, alpha)

    def check(dxa, dxb, outs):
        torch.cuda.synchronize()
        ra = norm_ref(xa.reshape(M, ca).to(DEV), ga.to(DEV), ba.to(DEV), "lrelu", dy=dya.reshape(M, ca).to(DEV))
        check_norm_bwd("pair A", M, ca, ra, dxa.reshape(M, ca), *outs[:3])
        se, ge = s.to(DEV).repeat_interleave(HW, 0), dgv.to(DEV).repeat_interleave(HW, 0)
        do = dob.reshape(M, cb).to(DEV)
        rb = norm_ref(xb.reshape(M, cb).to(DEV), gb.to(DEV), bb.to(DEV), "lrelu", 3, dy=mult * se * do + ge)
        mb = norm_ref(xb.reshape(M, cb).to(DEV), gb.to(DEV), bb.to(DEV), "lrelu", 3, dy=mult * se * do.abs() + ge.abs())
        for k in ("dxmag", "dxext", "dgmag", "dbmag", "dgext", "dbext"):
            rb[k] = mb[k]
        rb["kink"] = rb["kink"] | mb["kink"]
        check_norm_bwd("pair B", M, cb, rb, dxb[..., :cb].reshape(M, cb), *outs[3:])
        assert dxb[..., cb:].abs().max().item() == 0, "pad channels"
    return outputs, launch, check


LN_PAIR_KERNEL = {64: "ln_bwd_pair_kernel<8, 64, 1, false, 4, 10, 3, true>", 128: "ln_bwd_pair_kernel<16, 128, 1, false, 8, 21, 3, true>"}


@pytest.mark.parametrize("ca,cb", [(64, 30), (128, 63)], ids=["stage1", "stage2"])
def test_ln_pair(gen, ca, cb):
    """The shortcut norm (A) and conv2_bn with the re-weighting's backward (B) in one ln_bwd_pair_kernel launch; both bounded."""
    outputs, launch, check_pair = ln_pair_case(gen, ca, cb)
    bufs = outputs()
    ok, _ = routed(lambda: launch(*bufs), LN_PAIR_KERNEL[ca])
    assert ok
    check_pair(*bufs)


def test_norm_deferred_finish(gen):
    """Inside ops.overlap_region the partial rows go to the deferred workspace and one batched finish adds them at the end."""
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 9, 13, 37
    M, cp = B * H * W, 40
    x, dy = seam_data(gen, B, H, W, C), seam_data(gen, B, H, W, C)
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    dg, db, dbias = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    xd, dyd = to_dev(x)[1], to_dev(dy)[1]

    def run():
        with ops.overlap_region():
            return ops.norm_act_bwd(xd, dyd, C, padded(gamma, cp), padded(beta, cp), torch.empty_like(xd), dg, db, 0, 1, EPS, ops.ACT_ELU, 1.0,
                                    dbias=dbias)
    dx, got = routed(run, kname(True, 0, 1), "reduce_finish_batched_kernel")
    assert "reduce_finish_kernel" not in got, got
    torch.cuda.synchronize()
    ref = norm_ref(x.reshape(M, C).to(DEV), gamma.to(DEV), beta.to(DEV), "elu", dy=dy.reshape(M, C).to(DEV))
    check_norm_bwd("deferred", M, C, ref, dx[..., :C].reshape(M, C), dg, db, dbias)


@pytest.mark.parametrize("ca,cb,G", [(64, 30, 512), (128, 63, 256)], ids=["stage1", "stage2"])
def test_ln_pair_deferred_regions(gen, ca, cb, G):
    """The two partial-row regions of an ln_bwd_pair_kernel launch are reserved together.  Behind a first producer (64 floats), a
    deferral region of exactly their size holds A but not A and B, so the reservation flushes once and then places both; requesting B
    on its own after A would flush and put B at offset 0, across A (B > 64 floats).  G = workgroups of each role (one per 64-pixel tile,
    at most 512 at 4 per CU (stage 1: 38 KB of LDS) or 256 at 2 (stage 2: 54 KB), cardinal.hip launch_ln_pair); A = G*3*ca floats,
    B = G*3*roundup(cb, 8).  Every output equals the undeferred launch bit for bit (both finishes sum in reduce_finish_body's order)."""
    outputs, launch, check_pair = ln_pair_case(gen, ca, cb)
    ref = outputs()
    assert launch(*ref)
    got = outputs()
    na, nb = G * 3 * ca, G * 3 * ((cb + 7) // 8 * 8)
    assert na % 64 == 0 and nb > 64

    def run():
        with small_deferral(na + nb):
            assert launch(*got)
    _, names = routed(run, LN_PAIR_KERNEL[ca], "reduce_finish_batched_kernel")
    assert "reduce_finish_kernel" not in names, names      # both regions were deferred, none fell back to the caller's workspace
    torch.cuda.synchronize()
    for what, a, b in zip(("dxa", "dxb", "dgamma A", "dbeta A", "dbias A", "dgamma B", "dbeta B", "dbias B"), ref[:2] + tuple(ref[2]), got[:2] + tuple(got[2])):
        assert torch.equal(a, b), f"deferred pair: {what} differs from the undeferred launch"
    check_pair(*got)


# ------------------------------------------------------------------------------------------------ BN + act + 2x2 pool
@pytest.mark.parametrize("shape,C,act", [((2, 16, 32), 20, "lrelu"), ((2, 12, 20), 13, "elu"), ((1, 6, 34), 40, "relu")],
                         ids=["pow2", "div_12x20", "div_6x34"])
def test_bn_act_pool(gen, shape, C, act):
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    M, cp = B * H * W, (C + 7) // 8 * 8
    A, alpha = ACTS[act]
    x = seam_data(gen, B, H, W, C)
    dy = seam_data(gen, B, H // 2, W // 2, C)
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    mean, var = vec(gen, C, 0.0, 0.3), (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float().double()
    xd = to_dev(x)[1]
    G_, B_, M_, V_ = (padded(v, cp) for v in (gamma, beta, mean, var))
    obuf, od = nan_view(B, H // 2, W // 2, cp, cp + 8, 8)
    y, _ = routed(lambda: ops.bn_act_pool_fwd(xd, C, G_, B_, M_, V_, EPS, A, alpha, out=od), "bn_act_pool_kernel<false>")
    dg, db, dbias = torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV), torch.zeros(cp, device=DEV)
    dxbuf, dxd = nan_view(B, H, W, cp, cp + 16, 16)
    dx, _ = routed(lambda: ops.bn_act_pool_bwd(xd, to_dev(dy)[1], C, G_, B_, M_, V_, EPS, A, alpha, dxd, dg, db, dbias),
                   kname(True, 1, 1, pool=True), "reduce_finish_kernel")
    torch.cuda.synchronize()
    dyu = dy.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
    dev = lambda t: t.to(DEV)
    ref = norm_ref(x.reshape(M, C).to(DEV), dev(gamma), dev(beta), act, 1, 1, dev(mean), dev(var), dy=dyu.reshape(M, C).to(DEV))
    pool = lambda t: t.reshape(B, H // 2, 2, W // 2, 2, C).mean((2, 4))
    check(f"pool {shape} y", y[..., :C], pool(ref["y"]), pool(ref["ymag"]), U_BF16, 4.0)
    check_norm_bwd(f"pool {shape}", M, C, ref, dx[..., :C].reshape(M, C), dg, db, dbias)
    if cp > C:
        assert y[..., C:].abs().max().item() == 0 and dx[..., C:].abs().max().item() == 0, "pad channels"
    outside_untouched(obuf, 8, cp, "y")
    outside_untouched(dxbuf, 16, cp, "dx")


# ------------------------------------------------------------------------------------------------ BN batch statistics
def test_batchnorm_batch_statistics(gen):
    """Keras training-mode BN at M = 2^20 with |mean| / std of 0, 8, 30 and 100: the batch mean and variance, both moving
    statistics, y, dx, dgamma and dbeta.  (A one-pass variance sum x^2 / M - mean^2 in fp32 loses the variance to cancellation.)"""
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.flat import FlatParams
    from ultrasound_modeling_amd.layers import BatchNormalization
    B, H, W, C = 16, 256, 256, 8
    M = B * H * W
    std = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.25, 4.0, 2.0, 0.5], dtype=torch.float64)
    mu = torch.tensor([0.0, 8.0, 30.0, 100.0, 0.0, -8.0, -30.0, 100.0], dtype=torch.float64) * std
    g = torch.Generator(device=DEV).manual_seed(77)
    x = (torch.randn(M, C, generator=g, device=DEV, dtype=torch.float64) * std.to(DEV) + mu.to(DEV)).to(torch.bfloat16).double()
    dy = torch.randn(M, C, generator=g, device=DEV, dtype=torch.float64).to(torch.bfloat16).double()
    gamma, beta = vec(gen, C, neg=True), vec(gen, C, 0.0, 0.2)
    bn = BatchNormalization(C)
    bn.gamma.data.copy_(gamma)
    bn.beta.data.copy_(beta)
    FlatParams(bn, DEV)
    bn.training_mode = True
    xd = x.to(torch.bfloat16).reshape(B, H, W, C)
    y, _ = routed(lambda: bn.forward(xd, ops.ACT_LRELU, 0.3), "colsum_kernel<2>", "bn_batch_finalize_kernel", kname(False, 1, 1))
    dx, _ = routed(lambda: bn.backward(dy.to(torch.bfloat16).reshape(B, H, W, C)), kname(True, 1, 1), "bn_train_bwd_fix_kernel")
    torch.cuda.synchronize()
    ref = norm_ref(x, gamma.to(DEV), beta.to(DEV), "lrelu", mode="batch", dy=dy)
    mean, var = x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
    cf = c_f32(M)
    r1 = check("batch mean", bn._bmean[:C], mean, x.abs().mean(0), U_F32, cf)
    r2 = check("batch variance", bn._bvar[:C], var, var, U_F32, cf)
    mm, mv = ref["stats"]
    check("moving mean", bn.moving_mean, mm, 0.01 * x.abs().mean(0), U_F32, cf)
    check("moving variance", bn.moving_variance, mv, 0.99 + 0.01 * var, U_F32, cf)
    print(f"\n  batch statistics: worst ratios mean {r1:.3f}, variance {r2:.3f}", end="")
    check("batch y", y.reshape(M, C), ref["y"], ref["ymag"], U_BF16, 4.0)
    check_norm_bwd("batch", M, C, ref, dx.reshape(M, C), bn.gamma.grad, bn.beta.grad)


# ------------------------------------------------------------------------------------------------ split attention
# (id, B, H, W, P, R, radix (mult of the shared form; 0: distinct branches, mult 1), Cg, Hd, norm_mode, act, gap rows)
SA = [
    ("r1_sigmoid", 2, 6, 6, 2, 1, 1, 6, 3, 0, "lrelu", False),
    ("r1_radix2", 2, 4, 8, 3, 1, 2, 10, 5, 0, "lrelu", False),
    ("r1_radix3_cg85", 2, 3, 5, 3, 1, 3, 85, 42, 0, "lrelu", False),
    ("r1_radix4_p4", 2, 4, 4, 4, 1, 4, 8, 4, 0, "lrelu", False),
    ("r2_bn_elu", 2, 8, 8, 2, 2, 0, 32, 16, 1, "elu", False),
    ("r3_bn_elu_cg10", 2, 6, 6, 3, 3, 0, 10, 5, 1, "elu", False),
    ("r4_bn_elu", 2, 4, 4, 1, 4, 0, 16, 8, 1, "elu", False),
    ("r3_ln_lrelu", 1, 5, 7, 2, 3, 0, 12, 6, 0, "lrelu", False),
    ("limits_cg128_hd64", 2, 8, 8, 1, 1, 3, 128, 64, 0, "lrelu", False),
    ("limits_r4_cg128", 1, 4, 4, 1, 4, 0, 128, 64, 1, "elu", False),
    ("gap_rows", 2, 32, 32, 3, 1, 3, 10, 5, 0, "lrelu", True),
    ("gx8", 2, 64, 64, 3, 1, 3, 10, 5, 0, "lrelu", False),              # Cy 30: 64 pixels a trip, gx = 4096 / 512 = 8
    ("gx_cap64", 1, 256, 256, 3, 1, 3, 10, 5, 0, "lrelu", False),       # gx = 128 -> 64
    ("gx_cap_b32", 32, 128, 136, 3, 1, 3, 10, 5, 0, "lrelu", False),    # gx = 34 -> 1024 / 32 = 32
]


@pytest.mark.parametrize("B,H,W,P,R,radix,Cg,Hd,norm_mode,act,gap", [c[1:] for c in SA], ids=[c[0] for c in SA])
def test_split_attention(gen, B, H, W, P, R, radix, Cg, Hd, norm_mode, act, gap):
    from ultrasound_modeling_amd import ops
    HW = H * W
    mult = float(radix) if radix else 1.0
    sigmoid = (radix == 1) if radix else (R == 1)
    Cy, Co = P * R * Cg, P * Cg
    Cyp, Cop = (Cy + 7) // 8 * 8, (Co + 7) // 8 * 8
    A, alpha = ACTS[act]
    f = lambda *s, sc=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * sc).float().double()
    prm = [f(P, Cg, Hd, sc=1 / math.sqrt(Cg)), f(P, Hd, sc=0.1), 1 + f(P, Hd, sc=0.2), f(P, Hd, sc=0.1), f(P, Hd, sc=0.2),
           0.5 + torch.rand(P, Hd, generator=gen, dtype=torch.float64).float().double(), f(P, R, Hd, Cg, sc=1 / math.sqrt(Hd)), f(P, R, Cg, sc=0.1)]
    dev = lambda t: t.float().contiguous().to(DEV)
    params = tuple(dev(t) for t in prm)
    if norm_mode == 0:
        params = params[:4] + (None, None) + params[6:]
    y = seam_data(gen, B, H, W, Cy)
    dout = seam_data(gen, B, H, W, Co)
    gap_arg = None
    if gap:       # y and the pooled partial rows from the norm that feeds the block (nb > 1 rows per image)
        xd = to_dev(seam_data(gen, B, H, W, Cy))[1]
        yd, gap_arg = ops.norm_act_fwd_gap(xd, Cy, padded(vec(gen, Cy), Cyp), padded(vec(gen, Cy, 0.0, 0.2), Cyp), torch.empty_like(xd), 0, P,
                                           EPS, ops.ACT_LRELU, 0.3)
        assert gap_arg[1] > 1
        torch.cuda.synchronize()
        y = yd[..., :Cy].double().cpu()
    else:
        yd = to_dev(y)[1]
    obuf, od = nan_view(B, H, W, Cop, Cop + 16, 8)
    d = ops.splitattn_desc(B, HW, P, R, Cg, Hd, Cyp, Cop + 16, Cyp, Cop, mult, norm_mode, EPS, A, alpha, sigmoid)
    fwd_k = ("sa_mlp_kernel<false>", "sa_apply_kernel<false>") + (() if gap else ("sa_reduce_kernel",))
    (out, g, s, ws), _ = routed(lambda: ops.splitattn_fwd(d, yd, params, od, gap=gap_arg), *fwd_k)
    dbuf, dod = to_dev(dout, ld=Cop + 8, off=8, fill=NAN)
    grads = tuple(torch.zeros_like(t) for t in (params[0], params[1], params[2], params[3], params[6], params[7]))
    dyd = torch.full_like(yd, NAN)
    dy, _ = routed(lambda: ops.splitattn_bwd(d, yd, dod, params, grads, g, s, ws, dyd),
                   "sa_reduce_kernel", "sa_mlp_kernel<true>", "sa_apply_kernel<true>", "reduce_finish_kernel")
    torch.cuda.synchronize()

    r = sa_reference(y.reshape(B, HW, Cy).to(DEV), dout.reshape(B, HW, Co).to(DEV), [t.to(DEV) for t in prm], P, R, Cg, Hd, mult, norm_mode,
                     act, sigmoid)
    check(f"sa {B}x{HW} out", out[..., :Co].reshape(B, HW, Co), r["out"], r["outm"], U_BF16, 4.0)
    assert out[..., Co:].abs().max().item() == 0 if Cop > Co else True, "pad channels"
    outside_untouched(obuf, 8, Cop, "out")
    check(f"sa {B}x{HW} dy", dy[..., :Cy].reshape(B, HW, Cy), r["dy"], r["dym"], U_BF16, 4.0)
    if Cyp > Cy:
        assert dy[..., Cy:].abs().max().item() == 0, "pad channels"
    for nm, got, want, mag in zip(("dw1", "db1", "dgamma", "dbeta", "dw2", "db2"), grads, r["grads"], r["gmags"]):
        check(f"sa {B}x{HW} {nm}", got, want, mag, U_F32, c_f32(B * HW))
    outside_untouched(dbuf, 8, Cop, "dout")


@pytest.mark.parametrize("Cg,Hd,R", [(129, 8, 1), (8, 65, 1), (8, 4, 5)], ids=["cg129", "hd65", "r5"])
def test_split_attention_guard_limits(Cg, Hd, R):
    from ultrasound_modeling_amd import ops
    B, H, W, P = 1, 4, 4, 1
    Cy, Co = P * R * Cg, P * Cg
    Cyp, Cop = (Cy + 7) // 8 * 8, (Co + 7) // 8 * 8
    y = torch.zeros(B, H, W, Cyp, dtype=torch.bfloat16, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)
    params = (z(P, Cg, Hd), z(P, Hd), z(P, Hd), z(P, Hd), None, None, z(P, R, Hd, Cg), z(P, R, Cg))
    d = ops.splitattn_desc(B, H * W, P, R, Cg, Hd, Cyp, Cop, Cyp, Cop, 1.0, 0, EPS, ops.ACT_LRELU, 0.3, R == 1)
    out = torch.zeros(B, H, W, Cop, dtype=torch.bfloat16, device=DEV)
    no_launch(lambda: ops.splitattn_fwd(d, y, params, out))
    grads = (z(P, Cg, Hd), z(P, Hd), z(P, Hd), z(P, Hd), z(P, R, Hd, Cg), z(P, R, Cg))
    g, s, ws, dy = z(B, Cy), z(B, Cy), z(B * P * (Cg + 2 * Hd)), torch.empty_like(y)
    no_launch(lambda: ops.splitattn_bwd(d, y, out, params, grads, g, s, ws, dy))
