"""Pointwise / loss / optimiser route matrix (GPU): every route of the glue kernels of csrc/pointwise.hip and of the loss and optimiser
kernels of csrc/attn_loss_optim.hip, with a per-element bound.

Each case first asserts WHICH kernel it launched (route_probe.routed) and, through the launcher arithmetic restated in
tests/pointwise_restatement.py, the grid property it was chosen for (one partial workgroup / several with a ragged last trip / the grid
cap with a ragged end); then it checks every output element against an fp64 restatement built on the device from oracle/usseg_oracle.py
and the reference's Python (tests/pointwise_restatement.py, itself checked by tests/test_cpu_pointwise_restatement.py).  Inputs follow
route_probe.seam_data (one rare large element, a last image that is zero away from the seams, the last element of the tensor large).
Outputs are written into NaN-filled buffers, through channel-slice views where the entry point takes strides, and what lies outside the
view must still be NaN; pad channels are exact zeros where a kernel writes them.  Routes are driven by shapes only: USSEG_LOSS_PPT and the
other read-once switches are never set.

Bounds (|y - ref| <= c*u*mag + tiny for every element; U_BF16 = 2^-8, U_F32 = 2^-20, c = 4 for a bf16 output, c_f32(K) = 4 + sqrt(K)/8 for
an fp32 sum of K terms, tiny = 1e-6 unless stated (the optimiser rows, loss_cat_scale and the loss_kind 1 maps hold values far below 1e-6 and take a tiny of
1e-12, 2^-20/HW and 2^-20 * the largest scale instead); mag = the same operation on absolute values):
  * bitwise: copy_channels (plain), cast_input<float / double> (== x.float().to(bfloat16) on inputs that hold fp64 values just off an fp32
    tie of the bf16 rounding), cast_bf16_to_f32, space_to_depth2 both ways, reinject_hidden forward, fill.
  * act_fwd, act_bwd: bf16, c = 4, mag |act(x)|, |act'(x)*dy|, all four activations, no element left out (the inputs are bf16-exact, so the
    side of the kink is decided identically in either arithmetic).
  * copy_channels(accumulate), avgpool2_fwd, avgpool2_bwd (+ add), reinject_hidden backward: bf16, c = 4, mag = sum of |terms| (pool: mean |x|).
  * act_bwd_colsum, avgpool2_bwd_colsum: dx bitwise equal to act_bwd / avgpool2_bwd on the same operands; db against the fp64 column sum of
    the STORED bf16 dx, fp32, c_f32(M), mag = column sum of |dx| (+ what db held: the finishing launch ADDS to its destination).
  * colsum, channel_stats: fp32, c_f32(M), mag = column sum of |x|, of x^2 (+ what the destination held).
  * softmax probabilities: fp32, c_f32(C), mag p*(1 + |z - max z|).
  * dlogits: bf16, c = 4, mag[k] = p[k]*(|dLdp[k]| + sum_c |dLdp[c]|*p[c]), tiny = 2^-20 * inv_global_batch (times factor*max(w) for the
    class loss; loss_kind 1 applies no inv_global_batch: 2^-20 * the largest `scale`); pixels with an fp64 probability within 2^-20 relative
    of a clip constant are left out, counted, at most 0.1 %.  The forced rows [40, -40, 0, ...] (the first pixel and the last pixel of the last image) are not left out: their gradient is exactly 0.
  * scalar loss, loss map, loss_cat_scale: fp32, c_f32(K), K = the summed pixel terms, mag = sum of |terms|; ticket counter loss[1] == 0
    afterwards; a second call gives the same bits.  The scalar OVERWRITES loss[0] (grid_ordered_sum), as sumsq does with out[0].
  * sumsq: fp32, c_f32(n), mag = the fp64 sum; same bits on a second call and from sumsq_advance / sumsq_sched_advance.
  * adam, adamw: p, m, v after each of three steps: fp32, c = 4, mags |p| + |wd_t*p| + lr_t*|m'|/(sqrt(v') + eps), b1*|m| + (1-b1)*|g'|,
    b2*v + (1-b2)*g'^2.  The reference step is fed the kernel's own sumsq[0], lr_t and previous state, so the bound tests one update and not
    the norm (which has its own row).  scale_f32 the same way.
Each check prints its worst ratio err / bound (run with -s); test_zz_worst_ratio_table prints the worst per family and the file's wall time.

Routes, and the case that reaches each:
  * act_fwd_kernel, act_bwd_kernel, copy_channels_kernel: one partial workgroup, C = 8 (one chunk) and C = 520 (65 chunks) through strided
    views, past the 4096-block cap at M = 65539, C = 512 (test_act_fwd_bwd, test_copy_channels); act_fwd / act_bwd with the output
    aliasing an input, which holds only while every chunk is visited exactly once (test_act_in_place).
  * avgpool2_fwd_kernel (cap 4096*512 items), avgpool2_bwd_kernel with and without add: odd H/2 and W/2, B = 1, past both caps at
    258 x 510 x 512 (test_avgpool).
  * cast_input_kernel<float>, <double> (cap 4096*512), cast_bf16_f32_kernel (test_cast_input, test_cast_bf16_to_f32).
  * reinject_hidden_kernel forward and backward, n = 1, 3, 4 views of different c0 and ld, past its cap (test_reinject_hidden).
  * s2d_kernel<true>, <false> (test_space_to_depth2); fill_kernel (test_fill).
  * colsum_kernel<0> single slab (lanes per pixel 1..64, logical C below the padded width) and the slab route C = 520, 768, 1000 (last
    slab 488 wide), 3072 (cap 3072/6), 16384 (small M), each at one partial workgroup / a ragged four-row trip / the grid cap; refusals of
    C = 16385 and of an ld that is no multiple of 8; the deferred finish of a multi-slab launch (test_colsum*).
  * colsum_kernel<1> (test_channel_stats); act_bwd_colsum_kernel at the same C list (test_act_bwd_colsum); avgpool2_bwd_colsum_kernel at
    C = 8, 72, 512 and the wrapper's avgpool2_bwd_kernel + colsum_kernel<0> above 512 channels (test_avgpool_bwd_colsum*).
  * softmax_loss_kernel<3 | 0, false | true>: tail loop only (HW = 99), four-in-flight + tail (HW = 3109), 256 x 80, 256 x 256, B = 1 / 16,
    the g*nb > 2048 cap (B = 300), the map form and its 2048-block cap, the quad layout with the shift and the division decode, labels
    absent (test_softmax_loss).
  * loss_from_probs_kernel (kinds 0 and 1), loss_from_probs_cl_kernel (scalar and map), loss_cat_scale_kernel: one block and past their
    caps (test_loss_from_probs, test_loss_cat_scale).
  * sumsq_kernel, sumsq_sched_kernel (test_sumsq); adam_kernel, adamw_kernel (no decay, decay, masked decay with the scalar tail),
    scale_kernel (test_adam_steps, test_scale_by_clip); adam_kernel against the bits recorded from it in tests/golden
    (test_fixed_rate_step_keeps_the_recorded_bits).
Routes no shape reaches:
  * softmax_loss_pixel forms the quad pixel index (b*(H/2) + y/2)*(W/2) + x/2 in `int`: it overflows only from B*H*W/4 >= 2^31 quad pixels,
    i.e. more than 137 GB of fp32 logits in one call - not allocated here.
  * USSEG_LOSS_PPT other than 4 (an environment switch); M <= 0 / n <= 0 early returns (nothing is launched).
"""
import time

import numpy as np
import pytest
import torch

import loss_restatement as R
import pointwise_restatement as PR
import usseg_oracle as O
from route_probe import ACTS, TINY, U_BF16, U_F32, acheck, c_f32, nan_view, no_launch, outside_untouched, routed, small_deferral

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
BF = torch.bfloat16
B1, B2, EPS = (float(np.float32(v)) for v in (0.9, 0.999, 1e-7))       # the values the fp32 kernel arguments hold
T0 = time.time()
WORST = {}


def chk(family, what, y, ref, mag, u, c, tiny=TINY, keep=None):
    if keep is not None:
        y, ref, mag = y[keep], ref[keep], mag[keep]
    r = acheck(what, y, ref, mag, u, c, tiny=tiny)
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def dev_view(x, ld=None, off=0):
    """bf16 NHWC data -> (NaN-filled device buffer [B,H,W,ld], its view [..., off:off+roundup(C,8)] holding x and zero pad channels)."""
    B, H, W, C = x.shape
    cp = PR.roundup(C, 8)
    buf = torch.full((B, H, W, ld or cp), NAN, dtype=BF, device=DEV)
    v = buf[..., off:off + cp]
    v[..., :C] = x.to(DEV)
    if cp > C:
        v[..., C:] = 0
    return buf, v


def out_view(B, H, W, cp, view, slack=24, off=16):
    return nan_view(B, H, W, cp, cp + slack, off) if view else nan_view(B, H, W, cp, cp, 0)


def untouched(buf, off, cp, view, what):
    if view:
        outside_untouched(buf, off, cp, what)


def randn_bf(seed, *shape, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(*shape, device=DEV, generator=g) * scale).to(BF)
    rows = x.view(-1, shape[-1])               # seam_data's pattern over the rows: the second half zero away from the 16-row seams and the tail
    r = torch.arange(rows.shape[0], device=DEV)
    rows[(r >= rows.shape[0] // 2) & (r < rows.shape[0] - 2) & (r % 16 != 0) & (r % 16 != 15)] = 0
    x.view(-1)[-1] = 64 * scale
    x.view(-1)[0] = -48 * scale
    return x


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ elementwise walks
ACT_PARAMS = [(i, c, a) for i, c in enumerate(PR.ACT_CASES) for a in ACTS]


@pytest.mark.parametrize("i,case,act", ACT_PARAMS, ids=[f"{c[0]}-{a}" for _, c, a in ACT_PARAMS])
def test_act_fwd_bwd(i, case, act):
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, view = case
    for k in ("act_fwd", "act_bwd"):
        PR.walk_property(B * H * W * C // 8, PR.WALK_PER_THREAD[k], PR._walk_kind(cid))
    A, alpha = ACTS[act]
    x, dy = PR.seam_bf16(100 + i, B, H, W, C), PR.seam_bf16(200 + i, B, H, W, C)
    _, xd = dev_view(x, C + 16 if view else None, 8 if view else 0)
    _, dyd = dev_view(dy, C + 32 if view else None, 24 if view else 0)
    ybuf, yd = out_view(B, H, W, C, view)
    dxbuf, dxd = out_view(B, H, W, C, view, 8, 8)
    routed(lambda: ops.act_fwd(xd, yd, A, alpha), "act_fwd_kernel")
    routed(lambda: ops.act_bwd(xd, dyd, dxd, A, alpha), "act_bwd_kernel")
    x64, dy64 = xd.double(), dyd.double()
    chk("act_fwd", f"act_fwd {cid} {act}", yd, *PR.act_fwd_ref(x64, act), U_BF16, 4.0)
    chk("act_bwd", f"act_bwd {cid} {act}", dxd, *PR.act_bwd_ref(x64, dy64, act), U_BF16, 4.0)
    untouched(ybuf, 16, C, view, "y")
    untouched(dxbuf, 8, C, view, "dx")
    free()


@pytest.mark.parametrize("act", ["lrelu", "elu"])
@pytest.mark.parametrize("i,case", list(enumerate(PR.ACT_CASES)), ids=[c[0] for c in PR.ACT_CASES])
def test_act_in_place(i, case, act):
    """y aliasing x (and dx aliasing dy): safe only because the grid-stride walk visits every 16-byte chunk exactly once.  A walk that visits
    a chunk twice writes the same values out of place - no value check can see it - but applies the activation twice here."""
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, view = case
    A, alpha = ACTS[act]
    _, xd = dev_view(PR.seam_bf16(100 + i, B, H, W, C), C + 16 if view else None, 8 if view else 0)
    _, dyd = dev_view(PR.seam_bf16(200 + i, B, H, W, C), C + 32 if view else None, 24 if view else 0)
    x64, dy64 = xd.double(), dyd.double()
    routed(lambda: ops.act_bwd(xd, dyd, dyd, A, alpha), "act_bwd_kernel")
    chk("act_bwd", f"act_bwd in place {cid} {act}", dyd, *PR.act_bwd_ref(x64, dy64, act), U_BF16, 4.0)
    routed(lambda: ops.act_fwd(xd, xd, A, alpha), "act_fwd_kernel")
    chk("act_fwd", f"act_fwd in place {cid} {act}", xd, *PR.act_fwd_ref(x64, act), U_BF16, 4.0)
    free()


@pytest.mark.parametrize("i,case", list(enumerate(PR.ACT_CASES)), ids=[c[0] for c in PR.ACT_CASES])
def test_copy_channels(i, case):
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, view = case
    PR.walk_property(B * H * W * C // 8, PR.WALK_PER_THREAD["copy_channels"], PR._walk_kind(cid))
    _, src = dev_view(PR.seam_bf16(100 + i, B, H, W, C), C + 16 if view else None, 8 if view else 0)
    dbuf, dst = out_view(B, H, W, C, view)
    routed(lambda: ops.copy_channels(src, dst), "copy_channels_kernel")
    assert torch.equal(dst, src)
    untouched(dbuf, 16, C, view, "dst")
    dst.copy_(PR.seam_bf16(200 + i, B, H, W, C).to(DEV))
    d0 = dst.double()
    routed(lambda: ops.copy_channels(src, dst, accumulate=True), "copy_channels_kernel")
    chk("copy_channels(accumulate)", f"copy+= {cid}", dst, src.double() + d0, src.double().abs() + d0.abs(), U_BF16, 4.0)
    untouched(dbuf, 16, C, view, "dst")
    free()


@pytest.mark.parametrize("i,case", list(enumerate(PR.POOL_CASES)), ids=[c[0] for c in PR.POOL_CASES])
def test_avgpool(i, case):
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, view = case
    kind = PR._walk_kind(cid)
    PR.walk_property(B * (H // 2) * (W // 2) * C // 8, PR.WALK_PER_THREAD["avgpool2_fwd"], kind)
    PR.walk_property(B * H * W * C // 8, PR.WALK_PER_THREAD["avgpool2_bwd"], kind)
    _, xd = dev_view(PR.seam_bf16(300 + i, B, H, W, C), C + 16 if view else None, 8 if view else 0)
    _, dyd = dev_view(PR.seam_bf16(400 + i, B, H // 2, W // 2, C), C + 8 if view else None, 0)
    ybuf, yd = out_view(B, H // 2, W // 2, C, view)
    routed(lambda: ops.avgpool2_fwd(xd, yd), "avgpool2_fwd_kernel")
    chk("avgpool2_fwd", f"pool fwd {cid}", yd, *PR.pool_fwd_ref(xd.double()), U_BF16, 4.0)
    untouched(ybuf, 16, C, view, "y")
    for add in (None, xd):
        dxbuf, dxd = out_view(B, H, W, C, view, 8, 8)
        routed(lambda: ops.avgpool2_bwd(dyd, dxd, add), "avgpool2_bwd_kernel")
        chk("avgpool2_bwd", f"pool bwd {cid} add={add is not None}", dxd, *PR.pool_bwd_ref(dyd.double(), None if add is None else add.double()), U_BF16, 4.0)
        untouched(dxbuf, 8, C, view, "dx")
    free()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", PR.CAST_IN_CASES, ids=[c[0] for c in PR.CAST_IN_CASES])
def test_cast_input(case, dtype):
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, cp = case
    PR.walk_property(B * H * W * cp // 8, PR.WALK_PER_THREAD["cast_input"], PR._walk_kind(cid))
    x = PR.cast_ties((B, H, W, C), dtype)
    out, _ = routed(lambda: ops.cast_input(x.to(DEV), cp), "cast_input_kernel<double>" if dtype == torch.float64 else "cast_input_kernel<float>")
    want = x.float().to(BF)                    # Keras' autocast: the float32 value exists before the bf16 rounding
    assert torch.equal(out[..., :C].cpu().view(torch.int16), want.view(torch.int16))
    assert out[..., C:].abs().max().item() == 0
    free()


@pytest.mark.parametrize("shape,C,Cl,ld", [((2, 5, 7), 8, 5, 24), ((2, 9, 13), 24, 24, 24), ((1, 1, 65539), 512, 509, 512)], ids=["one_view", "few", "cap"])
def test_cast_bf16_to_f32(shape, C, Cl, ld):
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    PR.walk_property(B * H * W * Cl, PR.WALK_PER_THREAD["cast_bf16_to_f32"], {8: "one", 24: "few", 512: "cap"}[C])
    _, xd = dev_view(PR.seam_bf16(77, B, H, W, C), ld, ld - C)
    out, _ = routed(lambda: ops.to_f32(xd, Cl), "cast_bf16_f32_kernel")
    assert torch.equal(out, xd[..., :Cl].float())
    free()


@pytest.mark.parametrize("case", PR.REINJECT_CASES, ids=[c[0] for c in PR.REINJECT_CASES])
def test_reinject_hidden(case):
    from ultrasound_modeling_amd import ops
    cid, hshape, views = case
    n = int(np.prod(hshape))
    PR.walk_property(n // 8, PR.WALK_PER_THREAD["reinject_hidden"], PR._walk_kind(cid))
    hidden = randn_bf(500, *hshape)
    outs = [nan_view(*s[:3], s[3], ld, off) for s, ld, off in views]
    routed(lambda: ops.reinject_hidden(hidden, [v for _, v in outs], backward=False), "reinject_hidden_kernel")
    for (buf, v), (s, ld, off), ref in zip(outs, views, PR.reinject_fwd_ref(hidden, [s for s, _, _ in views])):
        assert torch.equal(v, ref), f"{cid}: view {s}"
        outside_untouched(buf, off, s[3], f"{cid} {s}")
    grads = []
    for k, (s, ld, off) in enumerate(views):
        buf = torch.full((*s[:3], ld), NAN, dtype=BF, device=DEV)
        buf[..., off:off + s[3]] = randn_bf(510 + k, *s)
        grads.append(buf[..., off:off + s[3]])
    dh = torch.full(hshape, NAN, dtype=BF, device=DEV)
    routed(lambda: ops.reinject_hidden(dh, grads, backward=True), "reinject_hidden_kernel")
    chk("reinject_hidden backward", f"reinject bwd {cid}", dh, *PR.reinject_bwd_ref([g.double() for g in grads], hshape), U_BF16, 4.0)
    free()


@pytest.mark.parametrize("case", PR.S2D_CASES, ids=[c[0] for c in PR.S2D_CASES])
def test_space_to_depth2(case):
    from ultrasound_modeling_amd import ops
    cid, (B, H, W), C, Np, ldf, ldq = case
    PR.walk_property(B * 4 * H * W * C // 8, PR.WALK_PER_THREAD["space_to_depth2"], PR._walk_kind(cid))
    same = lambda a, b: torch.equal(torch.nan_to_num(a.float(), nan=-7777.0), torch.nan_to_num(b.float(), nan=-7777.0))
    fbuf, full = dev_view(PR.seam_bf16(600, B, 2 * H, 2 * W, C), ldf, 0)
    qbuf = torch.full((B, H, W, ldq), NAN, dtype=BF, device=DEV)
    quad = qbuf[..., :4 * Np]
    routed(lambda: ops.space_to_depth2(full, quad, Np, to_quad=True), "s2d_kernel<true>")
    want = PR.s2d_ref(full, Np)
    assert same(quad, want), "to quad: a written slot differs or an unwritten one was touched"
    assert torch.isnan(qbuf[..., 4 * Np:].float()).all()
    back = torch.full((B, 2 * H, 2 * W, ldf), NAN, dtype=BF, device=DEV)
    routed(lambda: ops.space_to_depth2(back[..., :C], quad, Np, to_quad=False), "s2d_kernel<false>")
    assert torch.equal(back[..., :C], full) and torch.isnan(back[..., C:].float()).all()
    free()


@pytest.mark.parametrize("n", [1, 3, 4099, 4194304 + 3075])
def test_fill(n):
    from ultrasound_modeling_amd import ops
    assert (PR.cdiv(n, 1024) > 4096) == (n > 4194304)
    t = torch.full((n + 8,), NAN, device=DEV)
    routed(lambda: ops.fill_f32(t[:n], -2.5), "fill_kernel")
    assert (t[:n] == -2.5).all() and torch.isnan(t[n:]).all()


# ------------------------------------------------------------------------------------------------ column sums
def colsum_input(seed, M, C, view, zero_pads):
    cp = PR.roundup(C, 8)
    ld, off = (cp + 8, 8) if view else (cp, 0)
    buf = torch.full((1, 1, M, ld), NAN, dtype=BF, device=DEV)
    v = buf[..., off:off + cp]
    v.copy_(randn_bf(seed, 1, 1, M, cp))                    # colsum: the pad channels hold values, which must not reach db[:C]
    if zero_pads and cp > C:
        v[..., C:] = 0
    return v


def dst_vec(cp, C):
    d = torch.full((cp + 8,), 7.0, device=DEV)
    d[:C] = 0.5
    return d


@pytest.mark.parametrize("C,kind", PR.COLSUM_CASES, ids=[f"c{C}-{k}" for C, k in PR.COLSUM_CASES])
def test_colsum(C, kind):
    from ultrasound_modeling_amd import ops
    M, pl = PR.colsum_properties(C, kind)
    cp = PR.roundup(C, 8)
    xd = colsum_input(700 + C, M, C, C in (5, 72, 260, 1000, 3072), False)
    db = dst_vec(cp, C)
    routed(lambda: ops.colsum(xd, db, C), "colsum_kernel<0>", "reduce_finish_kernel")
    ref, mag = PR.colsum_ref(xd[..., :C].double().reshape(M, C))
    chk("colsum", f"colsum C{C} M{M} grid {pl['grid']}x{pl['nslab']}", db[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))
    assert (db[C:] == 7.0).all(), "db beyond C"
    free()


def test_colsum_refusals():
    from ultrasound_modeling_amd import ops
    db = torch.zeros(16392, device=DEV)
    wide = torch.zeros(1, 1, 4, 16392, dtype=BF, device=DEV)
    odd_ld = torch.zeros(1, 1, 4, 12, dtype=BF, device=DEV)
    no_launch(lambda: ops.colsum(wide[..., :16385], db, 16385))
    no_launch(lambda: ops.colsum(odd_ld[..., :8], db, 8))
    assert db.abs().max().item() == 0


@pytest.mark.parametrize("how", ["small_deferral", "overlap_region"])
def test_colsum_deferred_multi_slab(how):
    """The two slabs' partial rows of one launch go to the deferred region (behind another producer's 64 floats) and are finished by the
    batched kernel at the end: the same bits as the undeferred launch."""
    from ultrasound_modeling_amd import ops
    C = 1000
    M, pl = PR.colsum_properties(C, "few")
    xd = colsum_input(799, M, C, True, False)
    ref_db, db = dst_vec(C, C), dst_vec(C, C)
    ops.colsum(xd, ref_db, C)

    def run():
        if how == "small_deferral":
            with small_deferral(64 + pl["ws_floats"]):
                ops.colsum(xd, db, C)
        else:
            with ops.overlap_region():
                ops.colsum(xd, db, C)
    _, names = routed(run, "colsum_kernel<0>", "reduce_finish_batched_kernel")
    assert "reduce_finish_kernel" not in names, names
    torch.cuda.synchronize()
    assert torch.equal(db, ref_db)
    ref, mag = PR.colsum_ref(xd[..., :C].double().reshape(M, C))
    chk("colsum", f"colsum deferred {how}", db[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))


@pytest.mark.parametrize("C,kind", [c for c in PR.COLSUM_CASES if c[0] <= 512], ids=[f"c{C}-{k}" for C, k in PR.COLSUM_CASES if C <= 512])
def test_channel_stats(C, kind):
    from ultrasound_modeling_amd import ops
    M, pl = PR.colsum_properties(C, kind, slabs=False)
    cp = PR.roundup(C, 8)
    xd = colsum_input(800 + C, M, C, C in (5, 72), False)
    s, s2 = dst_vec(cp, C), dst_vec(cp, C)
    routed(lambda: ops.channel_stats(xd, C, s, s2), "colsum_kernel<1>", "reduce_finish_kernel")
    x64 = xd[..., :C].double().reshape(M, C)
    ref, mag = PR.colsum_ref(x64)
    chk("channel_stats sum", f"stats sum C{C} M{M}", s[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))
    ref, mag = PR.colsumsq_ref(x64)
    chk("channel_stats sumsq", f"stats sumsq C{C} M{M}", s2[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))
    assert (s[C:] == 7.0).all() and (s2[C:] == 7.0).all()
    free()


@pytest.mark.parametrize("j,C,kind", [(j, C, k) for j, (C, k) in enumerate(PR.COLSUM_CASES)], ids=[f"c{C}-{k}" for C, k in PR.COLSUM_CASES])
def test_act_bwd_colsum(j, C, kind):
    from ultrasound_modeling_amd import ops
    M, pl = PR.colsum_properties(C, kind)
    assert M % pl["stride"] != 0 or kind == "one"             # one row per trip: the last trip is ragged
    cp = PR.roundup(C, 8)
    act = list(ACTS)[j % 4]
    A, alpha = ACTS[act]
    view = C in (5, 72, 1000)
    xd, dyd = colsum_input(900 + C, M, C, view, True), colsum_input(950 + C, M, C, False, True)
    dxbuf, dxd = out_view(1, 1, M, cp, view, 8, 8)
    db = dst_vec(cp, C)
    routed(lambda: ops.act_bwd_colsum(xd, dyd, dxd, A, alpha, db, C), "act_bwd_colsum_kernel", "reduce_finish_kernel")
    dx2 = torch.full_like(xd, NAN)
    routed(lambda: ops.act_bwd(xd, dyd, dx2, A, alpha), "act_bwd_kernel")
    assert torch.equal(dxd, dx2), "dx differs from act_bwd"
    untouched(dxbuf, 8, cp, view, "dx")
    ref, mag = PR.colsum_ref(dxd[..., :C].double().reshape(M, C))
    chk("act_bwd_colsum db", f"act_bwd_colsum C{C} M{M} {act}", db[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))
    assert (db[C:] == 7.0).all(), "db beyond C"
    free()


@pytest.mark.parametrize("C,kind,add", PR.POOL_COLSUM_CASES, ids=[f"c{C}-{k}-{'add' if a else 'plain'}" for C, k, a in PR.POOL_COLSUM_CASES])
def test_avgpool_bwd_colsum(C, kind, add):
    from ultrasound_modeling_amd import ops
    B, H, W = PR.pool_colsum_shape(C, kind)
    M, pl = PR.colsum_properties(C, kind, rows=4, slabs=False, M=B * H * W)
    dyd = randn_bf(1000 + C, B, H // 2, W // 2, C)
    addd = randn_bf(1001 + C, B, H, W, C) if add else None
    dxbuf, dxd = nan_view(B, H, W, C, C + 8, 8)
    db = dst_vec(C, C)
    routed(lambda: ops.avgpool2_bwd(dyd, dxd, addd, db=db), "avgpool2_bwd_colsum_kernel", "reduce_finish_kernel")
    dx2 = torch.full((B, H, W, C), NAN, dtype=BF, device=DEV)
    routed(lambda: ops.avgpool2_bwd(dyd, dx2, addd), "avgpool2_bwd_kernel")
    assert torch.equal(dxd, dx2), "dx differs from avgpool2_bwd"
    outside_untouched(dxbuf, 8, C, "dx")
    ref, mag = PR.colsum_ref(dxd.double().reshape(M, C))
    chk("avgpool2_bwd_colsum db", f"pool_bwd_colsum C{C} M{M}", db[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(M))
    assert (db[C:] == 7.0).all()
    free()


def test_avgpool_bwd_colsum_above_512_channels():
    """Rows wider than the fused kernel's 512 channels: the wrapper runs the plain backward and a colsum launch, so db is still written."""
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 6, 10, 520
    dyd, addd = randn_bf(1100, B, H // 2, W // 2, C), randn_bf(1101, B, H, W, C)
    dxd = torch.full((B, H, W, C), NAN, dtype=BF, device=DEV)
    db = dst_vec(C, C)
    routed(lambda: ops.avgpool2_bwd(dyd, dxd, addd, db=db), "avgpool2_bwd_kernel", "colsum_kernel<0>", "reduce_finish_kernel")
    chk("avgpool2_bwd", "pool bwd C520", dxd, *PR.pool_bwd_ref(dyd.double(), addd.double()), U_BF16, 4.0)
    ref, mag = PR.colsum_ref(dxd.double().reshape(B * H * W, C))
    chk("avgpool2_bwd_colsum db", "pool_bwd + colsum C520", db[:C], ref + 0.5, mag + 0.5, U_F32, c_f32(B * H * W))
    assert (db[C:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ loss
def to_quad(l, fill):
    B, H, W, C = l.shape
    q = torch.full((B, H // 2, W // 2, 16), fill, dtype=l.dtype, device=l.device)
    for a in range(2):
        for b in range(2):
            q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + C] = l[:, a::2, b::2, :]
    return q


def from_quad(q):
    B, h, w, _ = q.shape
    out = torch.zeros(B, 2 * h, 2 * w, 4, dtype=q.dtype, device=q.device)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + 4]
    return out


@pytest.mark.parametrize("case", PR.LOSS_CASES, ids=[c[0] for c in PR.LOSS_CASES])
def test_softmax_loss(case):
    from ultrasound_modeling_amd import ops
    cid, kind, C, B, H, W, quad = case
    PR.loss_grid_properties(case)
    HW, M, inv = H * W, B * H * W, PR.loss_inv(B)
    logits, y = (t.to(DEV) for t in PR.loss_inputs(kind, C, B, H, W))
    r = PR.loss_ref(kind, C, logits, y, inv)
    if quad:
        lg = to_quad(logits.float(), NAN)
    else:
        lg = torch.full((B, H, W, 8 if C > 4 else 4), NAN, device=DEV)
        lg[..., :C] = logits.float()
    y32 = y.float()
    kw = dict(HW=HW, C_classes=C, inv_global_batch=inv, quad_w=W if quad else 0)
    tiny = 2.0 ** -20 * inv
    if kind == 1:
        scale = torch.full((H, W, C), NAN, device=DEV)
        ops.loss_cat_scale(y32, scale)
        kw.update(loss_kind=1, scale=scale)
        tiny = 2.0 ** -20 * r["scale"].max().item()
    elif kind == 2:
        w, gamma, factor = R.form(PR.LOSS_FORM, C)
        kw.update(class_loss=ops.class_loss(w, gamma, factor))
        tiny *= factor * max(w)
    name = f"softmax_loss_kernel<{3 if C == 3 else 0}, {'true' if kind == 2 else 'false'}>"

    def run():
        probs = torch.full((B, H, W, C), NAN, device=DEV)
        loss = torch.full((HW,), NAN, device=DEV) if kind == 1 else torch.zeros(ops.ACC_FLOATS, device=DEV)
        loss[0] = 123.0                                           # overwritten, not accumulated into
        dl = torch.full((B, H // 2, W // 2, 16) if quad else (B, H, W, 8), NAN, dtype=BF, device=DEV)
        routed(lambda: ops.softmax_loss(lg, y32, probs, loss, dl, **kw), name)
        return probs, loss, dl
    probs, loss, dl = run()
    chk("softmax probabilities", f"{cid} probs", probs, r["probs"], r["pmag"], U_F32, c_f32(C))
    if kind == 1:
        chk("loss map", f"{cid} map", loss.reshape(H, W), r["loss"], r["lossmag"], U_F32, c_f32(r["terms"]), tiny=tiny)
    else:
        chk("scalar loss", f"{cid} loss", loss[:1], r["loss"].reshape(1), r["lossmag"].reshape(1), U_F32, c_f32(M))
        assert loss[1].item() == 0, "ticket counter"
    d4 = from_quad(dl) if quad else dl
    assert not torch.isnan(d4.float()).any()
    if d4.shape[-1] > C:
        assert d4[..., C:].abs().max().item() == 0, "pad classes / pad slot of each 4-slot group"
    skip = r["edge"].clone()
    if kind != 1:
        for px in PR.forced_rows(B, H, W):
            assert r["dLdp"][px].abs().max().item() == 0 and d4[px].abs().max().item() == 0, f"the forced row {px}: exactly no gradient"
            skip[px] = False
    n_skip = int(skip.sum())
    print(f"\n  {cid}: {n_skip} of {M} pixels at a clip edge left out", end="")
    assert n_skip <= 1e-3 * M
    chk("dlogits", f"{cid} dlogits", d4[..., :C], r["dlogits"], r["mag"], U_BF16, 4.0, tiny=tiny, keep=~skip)
    p2, loss2, dl2 = run()
    assert torch.equal(p2, probs) and torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(dl2.view(torch.int16), dl.view(torch.int16)), \
        "a second call differs in its bits"
    # labels absent: the same probabilities, nothing else written
    p3 = torch.full_like(probs, NAN)
    loss3, dl3 = torch.full_like(loss, NAN), torch.full_like(dl, NAN)
    if kind == 2:       # the class-loss launcher refuses dlogits without labels before any launch, so dl3 is not handed over (and trivially stays NaN)
        no_launch(lambda: ops.softmax_loss(lg, None, p3, loss3, dl3, **kw))
    routed(lambda: ops.softmax_loss(lg, None, p3, loss3, None if kind == 2 else dl3, **kw), name)
    assert torch.equal(p3, probs) and torch.isnan(loss3).all() and torch.isnan(dl3.float()).all()
    free()


@pytest.mark.parametrize("case", PR.PROBS_CASES, ids=[c[0] for c in PR.PROBS_CASES])
def test_loss_from_probs(case):
    from ultrasound_modeling_amd import ops
    PR.probs_properties()
    cid, B, H, W = case
    HW, M, inv = H * W, B * H * W, 0.25
    p32, y32 = (t.to(DEV) for t in PR.probs_inputs(B, H, W))
    p, y = p32.double(), y32.double()
    acc = lambda: torch.cat([torch.tensor([123.0]), torch.zeros(ops.ACC_FLOATS - 1)]).to(DEV)
    # loss_kind 0
    loss = acc()
    routed(lambda: ops.loss_from_probs(p32, y32, loss, HW=HW, C_classes=3, inv_global_batch=inv), "loss_from_probs_kernel")
    want = O.compute_loss(y, p, 4)
    chk("scalar loss", f"probs {cid} kind 0", loss[:1], want.reshape(1), want.abs().reshape(1), U_F32, c_f32(M))
    assert loss[1].item() == 0
    again = acc()
    ops.loss_from_probs(p32, y32, again, HW=HW, C_classes=3, inv_global_batch=inv)
    assert same_bits(again[:2], loss[:2]), "kind 0: a second call differs in its bits"
    # loss_kind 1
    scale = torch.empty(H, W, 3, device=DEV)
    ops.loss_cat_scale(y32, scale)
    lmap = torch.full((HW,), NAN, device=DEV)
    routed(lambda: ops.loss_from_probs(p32, y32, lmap, HW=HW, C_classes=3, loss_kind=1, scale=scale), "loss_from_probs_kernel")
    want, mag = PR.loss_cat_map(y, p, PR.loss_cat_scale_ref(y))
    chk("loss map", f"probs {cid} kind 1", lmap.reshape(H, W), want, mag, U_F32, c_f32(3 * B), tiny=2.0 ** -20 * scale.max().item())
    again = torch.full((HW,), NAN, device=DEV)
    ops.loss_from_probs(p32, y32, again, HW=HW, C_classes=3, loss_kind=1, scale=scale)
    assert same_bits(again, lmap), "kind 1: a second call differs in its bits"
    # the class loss, scalar and map
    w, gamma, factor = R.form(PR.LOSS_FORM, 3)
    cl = ops.class_loss(w, gamma, factor)
    loss = acc()
    routed(lambda: ops.loss_from_probs(p32, y32, loss, HW=HW, C_classes=3, inv_global_batch=inv, class_loss=cl), "loss_from_probs_cl_kernel")
    want = R.scalar(y, p, w, gamma, factor, 4)
    chk("scalar loss", f"probs {cid} class loss", loss[:1], want.reshape(1), want.abs().reshape(1), U_F32, c_f32(M))
    assert loss[1].item() == 0
    again = acc()
    ops.loss_from_probs(p32, y32, again, HW=HW, C_classes=3, inv_global_batch=inv, class_loss=cl)
    assert same_bits(again[:2], loss[:2]), "class loss: a second call differs in its bits"
    lmap = torch.full((HW,), NAN, device=DEV)
    routed(lambda: ops.loss_from_probs(p32, y32, lmap, HW=HW, C_classes=3, inv_global_batch=inv, class_loss=cl, as_map=True), "loss_from_probs_cl_kernel")
    want = R.loss_map(y, p, w, gamma, factor)
    chk("loss map", f"probs {cid} class map", lmap.reshape(H, W), want, want.abs(), U_F32, c_f32(3 * B))
    again = torch.full((HW,), NAN, device=DEV)
    ops.loss_from_probs(p32, y32, again, HW=HW, C_classes=3, inv_global_batch=inv, class_loss=cl, as_map=True)
    assert same_bits(again, lmap), "class map: a second call differs in its bits"
    free()


@pytest.mark.parametrize("case", PR.SCALE_CASES, ids=[c[0] for c in PR.SCALE_CASES])
def test_loss_cat_scale(case):
    from ultrasound_modeling_amd import ops
    _id, B, H, W, C = case
    g = torch.Generator().manual_seed(5)
    y = torch.softmax(2 * torch.randn(B, H, W, C, generator=g), -1).to(DEV)
    scale = torch.full((H, W, C), NAN, device=DEV)
    routed(lambda: ops.loss_cat_scale(y, scale), "loss_cat_scale_kernel")
    ref = PR.loss_cat_scale_ref(y)
    chk("loss_cat_scale", f"loss_cat_scale {_id}", scale, ref, ref, U_F32, c_f32(B), tiny=2.0 ** -20 / (H * W))
    again = torch.full((H, W, C), NAN, device=DEV)
    ops.loss_cat_scale(y, again)
    assert same_bits(again, scale), "a second call differs in its bits"
    free()


# ------------------------------------------------------------------------------------------------ optimiser
def sched_table():
    t = np.zeros(48, dtype=np.int32)
    t[0] = 1
    t[16:17] = np.asarray([1e-3], dtype=np.float32).view(np.int32)
    return torch.from_numpy(t).to(DEV)


@pytest.mark.parametrize("n", PR.SUMSQ_N)
def test_sumsq(n):
    from ultrasound_modeling_amd import ops
    PR.optimiser_properties()
    gen = torch.Generator().manual_seed(n)
    buf = (torch.randn(n + 8, generator=gen) * 3).to(DEV)
    g = buf[4:4 + n]                                                # 16-byte aligned
    new = lambda: torch.cat([torch.tensor([123.0]), torch.zeros(ops.ACC_FLOATS - 1)]).to(DEV)
    out = new()
    routed(lambda: ops.sumsq(g, out), "sumsq_kernel")
    ref = (g.double() ** 2).sum().reshape(1)
    chk("sumsq", f"sumsq n={n}", out[:1], ref, ref, U_F32, c_f32(n))                  # out[0] = 123 was OVERWRITTEN
    assert out[1].item() == 0
    bits = lambda t: t[:1].view(torch.int32)
    o2 = new()
    ops.sumsq(g, o2)
    assert torch.equal(bits(o2), bits(out))
    step, lr_t, wd_t = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    o3 = new()
    routed(lambda: ops.sumsq_advance(g, o3, step, lr_t, 1e-3, B1, B2), "sumsq_kernel")
    o4 = new()
    routed(lambda: ops.sumsq_sched_advance(g, o4, step, sched_table(), lr_t, wd_t, B1, B2), "sumsq_sched_kernel")
    assert torch.equal(bits(o3), bits(out)) and torch.equal(bits(o4), bits(out)) and step.item() == 2
    assert o3[1].item() == 0 and o4[1].item() == 0
    no_launch(lambda: ops.sumsq(buf[1:1 + n], new()))               # g not 16-byte aligned
    free()


def clip_of(step):
    return (1.0, 1e9, 0.0)[step]          # clipped (the norm is far above 1); unclipped; no clipping at all


@pytest.mark.parametrize("n", PR.ADAM_N)
@pytest.mark.parametrize("variant", PR.ADAM_VARIANTS)
def test_adam_steps(variant, n):
    from ultrasound_modeling_amd import ops
    PR.optimiser_properties()
    p, g0, m, v, still = (t.to(DEV) for t in PR.optim_inputs(n))
    p0 = p.clone()
    mask = PR.decay_mask(n).to(DEV) if variant == "adamw_mask" else None
    wd = 3e-2 if variant in ("adamw_decay", "adamw_mask") else 0.0
    wd_t = torch.tensor([wd], dtype=torch.float32, device=DEV)
    twin = [t.clone() for t in (p, m, v)] if variant == "adamw_wd0" else None
    step, lr_t, ss = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.zeros(ops.ACC_FLOATS, device=DEV)
    for it in range(3):
        g = g0 * (1.0, 1e-3, 0.5)[it]
        clip = clip_of(it)
        ops.sumsq(g, ss)
        ops.adam_advance(step, lr_t, 1e-3, B1, B2)
        if it == 0:
            assert ss[0].item() > 1.0
        ref = PR.adam_ref(p, g, m, v, ss[0].item(), clip, lr_t.item(), wd_t.item(), mask, B1, B2, EPS)
        if variant == "adam":
            routed(lambda: ops.adam_clip_step(p, g, m, v, ss, clip, lr_t, B1, B2, EPS), "adam_kernel")
        else:
            routed(lambda: ops.adamw_step(p, g, m, v, ss, clip, lr_t, wd_t, mask, B1, B2, EPS), "adamw_kernel")
        fam = "adam" if variant == "adam" else "adamw"
        chk(f"{fam} p", f"{variant} n={n} step {it + 1} p", p, ref["p"], ref["pmag"], U_F32, 4.0, tiny=1e-12)
        chk(f"{fam} m", f"{variant} n={n} step {it + 1} m", m, ref["m"], ref["mmag"], U_F32, 4.0, tiny=1e-12)
        chk(f"{fam} v", f"{variant} n={n} step {it + 1} v", v, ref["v"], ref["vmag"], U_F32, 4.0, tiny=1e-12)
        if twin is not None:                      # adamw without decay == adam, bit for bit, past the grid cap too
            ops.adam_clip_step(twin[0], g, twin[1], twin[2], ss, clip, lr_t, B1, B2, EPS)
            for a, b, k in zip((p, m, v), twin, "pmv"):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"adamw(wd=0) != adam: {k} at n={n} step {it + 1}"
    assert step.item() == 3
    fixed = still if wd == 0.0 else (still & (mask == 0) if mask is not None else None)
    if fixed is not None:                         # zero gradient and zero moments: p keeps its bits, -0.0 included
        assert torch.equal(p[fixed].view(torch.int32), p0[fixed].view(torch.int32))
    free()


@pytest.mark.parametrize("n", [3, 4099])
def test_fixed_rate_step_keeps_the_recorded_bits(n):
    """tests/golden/adam_fixed_rate_bits.npz holds what the scalar adam_kernel gave on the GPU for the sequence of test_adam_steps("adam", n)
    (make_golden.py adam_fixed_rate_bits): n = 3 is one partial workgroup with n >> 2 == 0, n = 4099 several workgroups and a ragged end
    with the planted -0.0, zero-moment elements.  Every recorded array, step by step, bit for bit: the witness any later restatement of the
    fixed-rate step (one that shares adamw_elem with the table path, say) has to reproduce."""
    import os
    from ultrasound_modeling_amd import ops
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_fixed_rate_bits.npz"))
    dev = lambda k: torch.from_numpy(rec[f"n{n}::{k}"]).to(DEV)
    p, g0, m, v = (dev(k + "0") for k in "pgmv")
    assert all(same_bits(a, b.to(DEV)) for a, b in zip((p, g0, m, v), PR.optim_inputs(n)[:4])), "the fixture's inputs are optim_inputs(n)"
    step, lr_t, ss = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.zeros(ops.ACC_FLOATS, device=DEV)
    for it in range(3):
        g = g0 * (1.0, 1e-3, 0.5)[it]
        ops.sumsq(g, ss)
        ops.adam_advance(step, lr_t, 1e-3, B1, B2)
        routed(lambda: ops.adam_clip_step(p, g, m, v, ss, clip_of(it), lr_t, B1, B2, EPS), "adam_kernel")
        for k, t in zip("pmv", (p, m, v)):
            assert torch.equal(t.view(torch.int32), dev(f"step{it + 1}::{k}")), f"{k} differs from the recorded bits at n={n} step {it + 1}"
        assert same_bits(ss[:1], dev(f"step{it + 1}::sumsq")) and same_bits(lr_t, dev(f"step{it + 1}::lr_t")), f"sumsq / lr_t at n={n} step {it + 1}"
    free()


@pytest.mark.parametrize("n", PR.ADAM_N)
def test_scale_by_clip(n):
    from ultrasound_modeling_amd import ops
    g = PR.optim_inputs(n)[1].to(DEV)
    ss = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.sumsq(g, ss)
    g64 = g.double()
    routed(lambda: ops.scale_by_clip(g, ss, 1.0), "scale_kernel")
    scale = 1.0 / max(ss[0].item() ** 0.5, 1.0)
    assert scale < 1.0
    chk("scale_f32", f"scale n={n}", g, g64 * scale, g64.abs() * scale, U_F32, 4.0, tiny=1e-12)
    free()


def test_zz_worst_ratio_table():
    """Prints only (every check asserts on its own): the worst ratio per family over the cases that ran before it in this process."""
    print("\n  worst ratio err / bound per bounded output:")
    for k in sorted(WORST):
        print(f"    {k:32s} {WORST[k]:.3f}")
    print(f"  wall time of this file so far: {time.time() - T0:.1f} s")
