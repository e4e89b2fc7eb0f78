"""Float64 torch restatements of the glue, loss and optimiser operations behind csrc/pointwise.hip and csrc/attn_loss_optim.hip, written
after oracle/usseg_oracle.py and the reference's Python (ResNest.py, Decoder.py:140-141, VisionTransformer.py:205,225-227,244-245,
TBI_ResNest.py:234-248) - not after the kernels.  Every function returns the reference AND the magnitude `mag` (the same operation on
absolute values) that the per-element bound |y - ref| <= c*u*mag + tiny of tests/test_gpu_pointwise_routes.py uses.  All functions run on
the device of their arguments (the GPU tests build their references on the GPU, the CPU test on the host).

The second half restates, as plain Python, the grid every launcher chooses for a shape (grid_for, lanes_per_pixel, the slab count and cap
of usseg_colsum, softmax_loss_grid, the optimiser grids).  Kernel names are asserted through route_probe.routed; grid widths are not part
of a name, so a case asserts the property it was chosen for (grid == cap, the trips a thread takes, a ragged tail) through this arithmetic:
a case that stops reaching its route after a launcher change fails instead of silently testing less.

The third part holds the seeded input builders and the case tables, shared by the GPU tests and by tests/test_cpu_pointwise_restatement.py
(which checks on the very same inputs what the GPU tests rely on).
"""
import math

import torch

import loss_restatement as R
import usseg_oracle as O
from route_probe import act_d, act_f

BF16 = torch.bfloat16
CCE_EPS = O.KERAS["cce_clip"]
CCE_LS = O.KERAS["cce_label_smoothing"]
EDGE_REL = 2.0 ** -20


# ================================================================================================ restatements (fp64)
def act_fwd_ref(x, act):
    y = act_f(x, act)
    return y, y.abs()


def act_bwd_ref(x, dy, act):
    dx = act_d(x, act) * dy
    return dx, dx.abs()


def pool_fwd_ref(x):
    """2x2 average pool of NHWC x (ResNest.py:47 AveragePooling2D) -> (y, mean of |x|)."""
    B, H, W, C = x.shape
    v = x.reshape(B, H // 2, 2, W // 2, 2, C)
    return v.mean((2, 4)), v.abs().mean((2, 4))


def pool_bwd_ref(dy, add=None):
    """The pool's backward: every full-resolution pixel receives a quarter of its pooled pixel's gradient (+ the skip gradient `add`)."""
    up = dy.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
    if add is None:
        return up, up.abs()
    return up + add, up.abs() + add.abs()


def colsum_ref(x2d):
    return x2d.sum(0), x2d.abs().sum(0)


def colsumsq_ref(x2d):
    s = (x2d * x2d).sum(0)
    return s, s


def reinject_fwd_ref(hidden, shapes):
    """Decoder.py:140-141: the hidden state, row-major, seen as [B, h, w, c0] for every scale."""
    return [hidden.reshape(s) for s in shapes]


def reinject_bwd_ref(grads, hidden_shape):
    d = sum(g.reshape(hidden_shape) for g in grads)
    return d, sum(g.abs().reshape(hidden_shape) for g in grads)


def s2d_ref(full, Np):
    """full [B,2H,2W,C] -> quad [B,H,W,4*Np] with quad[b,i,j,(2a+b')*Np+n] = full[b,2i+a,2j+b',n]; unwritten slots are NaN."""
    B, H2, W2, C = full.shape
    q = torch.full((B, H2 // 2, W2 // 2, 4 * Np), float("nan"), dtype=full.dtype, device=full.device)
    for a in range(2):
        for b in range(2):
            q[..., (2 * a + b) * Np:(2 * a + b) * Np + C] = full[:, a::2, b::2, :]
    return q


def _dlogits_mag(p, dLdp):
    return p * (dLdp.abs() + (dLdp.abs() * p).sum(-1, keepdim=True))


def _softmax_parts(logits):
    z = logits.double().clone().requires_grad_(True)
    p = O.softmax_lastaxis(z)
    p.retain_grad()
    pmag = p.detach() * (1.0 + (z.detach() - z.detach().amax(-1, keepdim=True)).abs())
    return z, p, pmag


def cce_from_logits(logits, y, inv):
    """loss_kind 0: softmax -> O.compute_loss (label smoothing, division by the class sum, clip) with inv = 1/global_batch."""
    z, p, pmag = _softmax_parts(logits)
    per = O.cce_label_smoothing(y.double(), p)
    loss = per.sum() * inv
    loss.backward()
    pd = p.detach()
    q = pd / pd.sum(-1, keepdim=True)
    lo, hi = CCE_EPS, 1.0 - CCE_EPS
    edge = (((q - lo).abs() <= EDGE_REL * lo) | ((q - hi).abs() <= EDGE_REL * hi)).any(-1)
    return dict(probs=pd, pmag=pmag, loss=loss.detach(), lossmag=per.detach().abs().sum() * inv, dlogits=z.grad, dLdp=p.grad,
                mag=_dlogits_mag(pd, p.grad), edge=edge, terms=per.numel())


def loss_cat_scale_ref(y):
    """TBI_ResNest.py:240-241 for every class: scale[h,w,c] = 1/(sum_b y + 1)/(H*W)."""
    HW = y.shape[1] * y.shape[2]
    return 1.0 / (y.double().sum(0) + 1.0) / HW


def loss_cat_map(y, p, scale):
    """TBI_ResNest.py:244-246 for any class count: -sum_b sum_c y*log(p + 1e-7)*scale -> ([H,W] map, the sum of |terms|)."""
    t = y.double() * torch.log(p + 1e-7) * scale
    return -t.sum((0, 3)), t.abs().sum((0, 3))


def cat_from_logits(logits, y):
    """loss_kind 1: softmax -> my_loss_cat's [H,W] map; the gradient is that of the map's sum."""
    z, p, pmag = _softmax_parts(logits)
    scale = loss_cat_scale_ref(y)
    lmap, lmag = loss_cat_map(y, p, scale)
    lmap.sum().backward()
    pd = p.detach()
    return dict(probs=pd, pmag=pmag, loss=lmap.detach(), lossmag=lmag.detach(), dlogits=z.grad, dLdp=p.grad, mag=_dlogits_mag(pd, p.grad),
                edge=torch.zeros(pd.shape[:-1], dtype=torch.bool, device=pd.device), scale=scale, terms=y.shape[0] * y.shape[3])


def class_from_logits(logits, y, w, gamma, factor, inv):
    """loss_kind 2 through tests/loss_restatement.py (every term of that loss is >= 0, so its mag is the loss itself)."""
    r = R.from_logits(logits, y, w, gamma, factor, inv)
    zz = logits.double()
    r["pmag"] = r["probs"] * (1.0 + (zz - zz.amax(-1, keepdim=True)).abs())
    r["lossmag"] = r["loss"].abs()
    r["terms"] = r["probs"][..., 0].numel()
    return r


def adam_ref(p, g, m, v, sumsq, clip_norm, lr_t, wd_t=0.0, mask=None, b1=0.9, b2=0.999, eps=1e-7):
    """One clipped Adam / AdamW step in fp64 (O.clip_by_global_norm given sum g^2, tfa's decoupled decay p -= wd_t*p where `mask`,
    O.adam_step given lr_t).  -> p', m', v' and their mags."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    scale = clip_norm / max(math.sqrt(sumsq), clip_norm) if clip_norm > 0 else 1.0
    gs = g * scale
    dec = wd_t * p
    if mask is not None:
        dec = dec * (mask != 0).to(p.dtype)
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    upd = lr_t * m1 / (v1.sqrt() + eps)
    return dict(p=p - dec - upd, m=m1, v=v1, pmag=p.abs() + dec.abs() + upd.abs(), mmag=b1 * m.abs() + (1.0 - b1) * gs.abs(), vmag=v1,
                scale=scale)


def lr_t_ref(step, lr, b1=0.9, b2=0.999):
    return lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


# ================================================================================================ the launchers' grids
REDUCE_MAX_BLOCKS = 1024


def cdiv(a, b):
    return -(-a // b)


def roundup(a, b):
    return cdiv(a, b) * b


def lanes_per_pixel(chunks):
    l = 1
    while l < chunks:
        l <<= 1
    return l


def grid_for(work, per_block, cap=2048):
    return max(1, min(cdiv(work, per_block), cap))


def walk(items, per_thread, cap=4096):
    """An elementwise grid-stride walk of `items` 16-byte (or scalar) items: grid, the most trips a thread takes, whether the last trip is
    ragged (some threads of the grid idle in it) and whether the grid sits at its cap."""
    g = grid_for(items, 256 * per_thread, cap)
    return dict(grid=g, trips=cdiv(items, g * 256), ragged=items % (g * 256) != 0, capped=cdiv(items, 256 * per_thread) > cap,
                at_cap=g == cap)


WALK_PER_THREAD = dict(act_fwd=4, act_bwd=4, copy_channels=4, avgpool2_fwd=2, avgpool2_bwd=4, cast_input=2, cast_bf16_to_f32=4,
                       reinject_hidden=2, space_to_depth2=4, fill=4, scale=4, adam=4)


def colsum_plan(M, C, rows_per_block_trip=8, slabs=True):
    """usseg_colsum / usseg_act_bwd_colsum (slabs) and usseg_channel_stats / usseg_avgpool2_bwd_colsum (one slab, C <= 512)."""
    nslab = cdiv(C, 512) if slabs else 1
    cwp = 512 if nslab > 1 else roundup(C, 8)
    lpp = lanes_per_pixel(cwp // 8)
    ppb = 4 * (64 // lpp)
    cap = min(REDUCE_MAX_BLOCKS * 3 // nslab, REDUCE_MAX_BLOCKS)
    grid = grid_for(M, ppb * rows_per_block_trip, cap)
    return dict(nslab=nslab, cwp=cwp, lpp=lpp, ppb=ppb, cap=cap, grid=grid, stride=grid * ppb, last_slab=C - (nslab - 1) * 512,
                ws_floats=grid * nslab * cwp)


def colsum_M(C, kind, slabs=True, rows=8):
    """The three row counts of a column-sum case: 'one' partial workgroup, 'few' workgroups with a ragged four-row trip, past the 'cap'."""
    pl = colsum_plan(1, C, rows, slabs)
    ppb, cap = pl["ppb"], pl["cap"]
    return {"one": ppb + 3, "few": ppb * rows * 5 - ppb + 7, "cap": cap * ppb * rows + 4 * cap * ppb + ppb + 1}[kind]


def softmax_loss_grid(HW, nb, map_form, ppt=4):
    if map_form:
        return min(cdiv(HW, 256), 2048), 1
    g = cdiv(HW, 256 * ppt)
    if g * nb > 2048:
        g = max(2048 // nb, 1)
    assert g * nb <= 2048
    return g, nb


def softmax_loss_trips(HW, gx):
    """(threads that run the four-in-flight loop at least once, threads that run the single-pixel tail loop, is the tail ragged)"""
    stride = gx * 256
    hw0 = torch.arange(stride)
    n4 = ((HW - 3 * stride - hw0).clamp(min=0) + 4 * stride - 1) // (4 * stride)          # trips of `for (; hw + 3*stride < HW; hw += 4*stride)`
    left = (HW - (hw0 + 4 * stride * n4)).clamp(min=0)
    nt = (left + stride - 1) // stride                                                       # trips of the tail loop
    return dict(stride=stride, four=int((n4 > 0).sum()), tail=int((nt > 0).sum()), both=int(((n4 > 0) & (nt > 0)).sum()),
                ragged=bool((nt.max() != nt.min()) or (n4.max() != n4.min())))


def loss_from_probs_grid(M, HW, as_map):
    return min(cdiv(HW, 256) if as_map else cdiv(M, 1024), 2048)


def loss_cat_scale_grid(HW, C):
    return min(cdiv(HW * C, 256), 2048)


def sumsq_grid(n):
    return min(cdiv(n, 4096), 256)


def adam_grid(n):
    return min(cdiv(n, 1024), 4096)


def adamw_grid(n):
    return min(cdiv(max(n >> 2, 1), 256), 4096)


# ================================================================================================ inputs and case tables
def seam_bf16(seed, B, H, W, C, scale=1.0):
    """route_probe.seam_data's pattern as a bf16 tensor (built in fp32, so that the 67M-element cases need no fp64 host copy): one rare large
    element, a last image that is zero away from the 16-row seams, the last element of the tensor large."""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, H, W, C, generator=gen, dtype=torch.float32) * scale).to(BF16)
    if B > 1 and H > 4:
        keep = torch.tensor([r % 16 in (0, 15) or r >= H - 2 for r in range(H)])
        x[B - 1, ~keep] = 0
    x[B - 1, H - 1, W - 1, C - 1] = 64 * scale
    x[0, H // 2, 0, 0] = -48 * scale
    return x


# (id, (B, H, W), C, view): M*C/8 items.  one: a single partial workgroup; few: several with a ragged last trip; cap: past 4096 blocks
ACT_CASES = [
    ("one_c24", (1, 7, 9), 24, False),
    ("one_c8_view", (2, 5, 7), 8, True),
    ("few_c520_view", (2, 9, 13), 520, True),
    ("cap_c512", (1, 1, 65539), 512, False),
]
# avgpool: (id, (B, H, W) of the full-resolution tensor, C, view)
POOL_CASES = [
    ("one_b1_odd", (1, 6, 10), 24, True),
    ("one_c8", (2, 2, 6), 8, False),
    ("few_c520_odd", (2, 18, 26), 520, True),
    ("cap_c512_odd", (1, 258, 510), 512, False),
]
CAST_IN_CASES = [("one_c3", (2, 5, 7), 3, 8), ("few_c10", (2, 19, 23), 10, 16), ("cap_c1", (1, 1449, 1449), 1, 8)]
# reinject: (id, hidden shape, [(view shape, ld, channel offset)])
REINJECT_CASES = [
    ("n1_one", (1, 5, 64), [((1, 5, 8, 8), 16, 8)]),
    ("n4_one", (1, 5, 64), [((1, 1, 5, 64), 72, 8), ((1, 4, 5, 16), 16, 0), ((1, 5, 8, 8), 24, 16), ((1, 2, 5, 32), 48, 8)]),
    ("n3_few", (2, 81, 64), [((2, 9, 9, 64), 64, 0), ((2, 18, 18, 16), 32, 8), ((2, 36, 18, 8), 16, 8)]),
    ("n3_cap", (1, 32776, 512), [((1, 16, 8194, 128), 136, 8), ((1, 64, 8194, 32), 40, 0), ((1, 256, 8194, 8), 16, 8)]),
]
# s2d: (id, (B, H, W) of the quad map, C, Np, ld_full, ld_quad)
S2D_CASES = [("one", (2, 3, 5), 8, 16, 16, 72), ("few", (2, 9, 13), 24, 24, 32, 96), ("cap", (1, 129, 255), 256, 264, 256, 1056)]

COLSUM_C_ONE = [5, 8, 24, 72, 260, 512]
COLSUM_C_SLAB = [520, 768, 1000, 3072, 16384]
COLSUM_CASES = [(C, k) for C in COLSUM_C_ONE + COLSUM_C_SLAB for k in ("one", "few", "cap") if not (C == 16384 and k == "cap")]
POOL_COLSUM_CASES = [(C, k, add) for C in (8, 72, 512) for k in ("one", "few", "cap") for add in (False, True)]

# softmax_loss: (id, loss_kind, C, B, H, W, quad)
LOSS_CASES = [
    ("k0_c3_hw99", 0, 3, 2, 9, 11, False),
    ("k0_c2_four_and_tail_b1", 0, 2, 1, 1, 3109, False),
    ("k0_c3_four_and_tail_b16", 0, 3, 16, 1, 3109, False),
    ("k2_c4_256x80", 2, 4, 2, 256, 80, False),
    ("k0_c8_256x80_b1", 0, 8, 1, 256, 80, False),
    ("k0_c3_256x256_b16", 0, 3, 16, 256, 256, False),
    ("k2_c3_256x256_b1", 2, 3, 1, 256, 256, False),
    ("k2_c8_hw99", 2, 8, 2, 9, 11, False),
    ("k0_c3_cap_b300", 0, 3, 300, 64, 128, False),
    ("k2_c2_cap_b300", 2, 2, 300, 64, 128, False),
    ("k1_c3_hw99", 1, 3, 2, 9, 11, False),
    ("k1_c3_256x80_b16", 1, 3, 16, 256, 80, False),
    ("k1_c8_tail_b1", 1, 8, 1, 1, 3109, False),
    ("k1_c2_256x256", 1, 2, 2, 256, 256, False),
    ("k1_c4_mapcap_b3", 1, 4, 3, 1024, 514, False),
    ("quad_k0_c3_w64_shift", 0, 3, 2, 32, 64, True),
    ("quad_k2_c4_w256_shift", 2, 4, 1, 256, 256, True),
    ("quad_k0_c3_w80_div", 0, 3, 2, 256, 80, True),
    ("quad_k0_c4_w6_div", 0, 4, 2, 10, 6, True),
    ("quad_k2_c3_w6_div", 2, 3, 3, 6, 6, True),
    ("quad_k1_c3_w80_div", 1, 3, 2, 256, 80, True),
]
LOSS_FORM = "weighted_focal"        # the class-loss form of the loss_kind 2 cases (all three forms: tests/test_gpu_class_loss.py)
# loss_from_probs: (id, B, H, W): one block; M past 2048*1024 pixels with HW past the map cap of 2048*256
PROBS_CASES = [("one_block", 3, 9, 11), ("past_caps", 3, 1, 700001)]
SCALE_CASES = [("small", 2, 9, 11, 3), ("past_cap", 3, 1024, 514, 4)]

SUMSQ_N = [1, 3, 4, 7, 4099, 1048576, 1048576 + 4097, 5000003]
ADAM_N = [3, 4099, 4194304 + 3075, 5000003]
ADAM_VARIANTS = ["adam", "adamw_wd0", "adamw_decay", "adamw_mask"]


# ---- the property each case was chosen for (asserted by the CPU test and again by the GPU case that relies on it)
def _walk_kind(cid):
    return "cap" if "cap" in cid else ("few" if "few" in cid else "one")


def walk_property(items, per_thread, kind):
    w = walk(items, per_thread)
    if kind == "one":
        assert w["grid"] == 1 and items % 256 != 0, (items, w)
    elif kind == "few":
        assert 1 < w["grid"] < 4096 and w["ragged"] and w["trips"] >= 2, (items, w)
    else:
        assert w["capped"] and w["grid"] == 4096 and w["ragged"] and items > 4096 * 256 * per_thread, (items, w)
    return w


def walk_properties():
    for cid, (B, H, W), C, _v in ACT_CASES:
        for k in ("act_fwd", "act_bwd", "copy_channels"):
            walk_property(B * H * W * C // 8, WALK_PER_THREAD[k], _walk_kind(cid))
    walk_property(65539 * 509, WALK_PER_THREAD["cast_bf16_to_f32"], "cap")
    for cid, (B, H, W), C, _v in POOL_CASES:
        walk_property(B * (H // 2) * (W // 2) * C // 8, WALK_PER_THREAD["avgpool2_fwd"], _walk_kind(cid))
        walk_property(B * H * W * C // 8, WALK_PER_THREAD["avgpool2_bwd"], _walk_kind(cid))
        assert "odd" not in cid or ((H // 2) % 2 == 1 and (W // 2) % 2 == 1)
    for cid, (B, H, W), C, cp in CAST_IN_CASES:
        walk_property(B * H * W * cp // 8, WALK_PER_THREAD["cast_input"], _walk_kind(cid))
    for cid, hshape, views in REINJECT_CASES:
        n = math.prod(hshape)
        walk_property(n // 8, WALK_PER_THREAD["reinject_hidden"], _walk_kind(cid))
        for shape, ld, off in views:
            assert math.prod(shape) == n and shape[3] % 8 == 0 and ld % 8 == 0 and off % 8 == 0 and ld >= off + shape[3]
    for cid, (B, H, W), C, Np, ldf, ldq in S2D_CASES:
        walk_property(B * 4 * H * W * C // 8, WALK_PER_THREAD["space_to_depth2"], _walk_kind(cid))
        assert Np >= C and ldf >= C and ldq >= 4 * Np


def colsum_properties(C, kind, rows=8, slabs=True, M=None):
    """-> (M, plan) of a column-sum case, with the property it was chosen for asserted.  `rows`: the rows a workgroup is sized for (8: colsum,
    act_bwd_colsum, channel_stats, whose loops take four rows or one row per trip; 4: avgpool2_bwd_colsum, one row per trip)."""
    M = colsum_M(C, kind, slabs, rows) if M is None else M
    pl = colsum_plan(M, C, rows, slabs)
    four = 4 if rows == 8 else 1
    if kind == "one":
        assert pl["grid"] == 1 and M < rows * pl["ppb"], (M, pl)
    elif kind == "few":
        assert 1 < pl["grid"] < pl["cap"] and M % (four * pl["stride"]) != 0 and M % pl["stride"] != 0 and M > four * pl["stride"], (M, pl)
    else:
        assert pl["grid"] == pl["cap"] and cdiv(M, pl["ppb"] * rows) > pl["cap"], (M, pl)
        assert M % (four * pl["stride"]) != 0 and M % pl["stride"] != 0 and M > four * pl["stride"], (M, pl)
    assert pl["ws_floats"] <= REDUCE_MAX_BLOCKS * 3 * 512                      # usseg_reduce_ws_floats
    return M, pl


def pool_colsum_shape(C, kind):
    """(B, H, W) of the full-resolution gradient of an avgpool2_bwd_colsum case (H and W even, so M is a multiple of 4)."""
    B, H = {"one": (1, 2), "few": (3, 6), "cap": (2, 128)}[kind]
    W = 2 * cdiv(colsum_M(C, kind, False, 4), B * H * 2)
    return B, H, W


def loss_grid_properties(case):
    """The grid property each softmax_loss case was chosen for -> the grid of the labelled launch."""
    cid, kind, C, B, H, W, quad = case
    HW = H * W
    grid = gx, gy = softmax_loss_grid(HW, B, kind == 1)
    if kind == 1:
        assert gy == 1
        if "mapcap" in cid:
            assert HW > 2048 * 256 and gx == 2048 and HW % (2048 * 256) != 0
        gx, gy = softmax_loss_grid(HW, B, False)            # without labels a loss_kind 1 call takes the (pixel blocks, images) grid
    t = softmax_loss_trips(HW, gx)
    if "hw99" in cid:
        assert gx == 1 and t["four"] == 0 and t["tail"] == 99
    if "four_and_tail" in cid or "tail_b1" in cid:
        assert HW == 256 * 4 * 3 + 37 and 0 < t["four"] < t["stride"] and t["tail"] > 0 and t["ragged"]
    if "cap_b300" in cid:
        assert cdiv(HW, 1024) * B > 2048 and gx == 2048 // B == 6 and gy == B and t["four"] == t["stride"] and t["ragged"]
    if "256x256_b16" in cid:
        assert gx * gy == 1024 and t["four"] == t["stride"] and t["tail"] == 0
    if quad:
        assert W % 2 == 0 and H % 2 == 0 and C <= 4 and ("shift" in cid) == (W & (W - 1) == 0)
    return grid


def optimiser_properties():
    assert [sumsq_grid(n) for n in SUMSQ_N] == [1, 1, 1, 1, 2, 256, 256, 256]
    assert cdiv(1048576, 4096) == 256 and cdiv(1048576 + 4097, 4096) > 256 and 5000003 % 4 == 3          # the cap reached exactly; past it
    assert [n >> 2 for n in SUMSQ_N[:3]] == [0, 0, 1]                                                     # n < 4: the scalar tail alone
    for n, capped in zip(ADAM_N, (False, False, True, True)):
        assert (cdiv(n, 1024) > 4096) == capped == (n > 4194304) and (adam_grid(n) == 4096) == capped
        assert (cdiv(max(n >> 2, 1), 256) > 4096) == capped and (adamw_grid(n) == 4096) == capped
        assert n % 4 == 3                                                                                 # every size has a scalar tail


def probs_properties():
    for cid, B, H, W in PROBS_CASES:
        M = B * H * W
        if cid == "one_block":
            assert loss_from_probs_grid(M, H * W, False) == 1 == loss_from_probs_grid(M, H * W, True)
        else:
            assert M > 2048 * 1024 and H * W > 2048 * 256 and loss_from_probs_grid(M, H * W, False) == 2048 == loss_from_probs_grid(M, H * W, True)
    (_s, B, H, W, C), (_c, B2, H2, W2, C2) = SCALE_CASES
    assert loss_cat_scale_grid(H * W, C) < 2048 == loss_cat_scale_grid(H2 * W2, C2) and (H2 * W2 * C2) % (2048 * 256) != 0


def forced_rows(B, H, W):
    """The pixels whose logits are forced to [40, -40, 0, ...]: the first one (thread 0 of the first workgroup, first trip) and the last pixel
    of the last image (the ragged tail of the last workgroup)."""
    return [(0, 0, 0), (B - 1, H - 1, W - 1)]


def loss_inputs(kind, C, B, H, W):
    """fp32-exact logits 2*randn with the rows of forced_rows() forced to [40, -40, 0, ...] (clipped on every class by orders of magnitude), and soft
    labels.  (At 3*randn and two classes, 0.1 % of the pixels saturate to within 2^-20 of the upper clip constant: the edge set's whole allowance.)"""
    gen = torch.Generator().manual_seed(9000 + 97 * kind + 13 * C + B + H * W)
    logits = (torch.randn(B, H, W, C, generator=gen, dtype=torch.float32) * 2).double()
    for px in forced_rows(B, H, W):
        logits[px] = torch.tensor([40.0, -40.0] + [0.0] * (C - 2), dtype=torch.float64)[:C]
    y = torch.softmax(2 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float32), -1).double()
    return logits, y


def loss_ref(kind, C, logits, y, inv):
    if kind == 0:
        return cce_from_logits(logits, y, inv)
    if kind == 1:
        return cat_from_logits(logits, y)
    return class_from_logits(logits, y, *R.form(LOSS_FORM, C), inv)


def loss_inv(B):
    return 1.0 / (B + 2)


def probs_inputs(B, H, W, C=3):
    """Un-normalised fp32 probabilities (both clip constants present) and soft labels."""
    gen = torch.Generator().manual_seed(77 + B * H * W)
    p = torch.softmax(3 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float32), -1)
    p[0, 0, 0] = torch.tensor([1.0, 0.0, 0.0])
    p = (p * (0.5 + torch.rand(B, H, W, 1, generator=gen))).clamp(max=1.0)
    y = torch.softmax(2 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float32), -1)
    return p, y


def optim_inputs(n, seed=5):
    """p, g, m, v (fp32) of one flat parameter vector; the first 1/16 of every 4096 has zero gradient and zero moments, with p = -0.0 on the
    even ones of those."""
    gen = torch.Generator().manual_seed(seed + n)
    p, g, m = (torch.randn(n, generator=gen) * s for s in (0.1, 5.0, 0.05))
    v = torch.rand(n, generator=gen) * 1e-3
    idx = torch.arange(n)
    still = (idx % 4096) < 256
    if n < 8:
        still = idx == 1
    g[still], m[still], v[still] = 0.0, 0.0, 0.0
    p[still & (idx % 2 == 0)] = -0.0
    return p, g, m, v, still


def decay_mask(n):
    """uint8 decay mask whose set bits include the scalar tail n - (n % 4) .. n - 1."""
    gen = torch.Generator().manual_seed(31 + n)
    k = (torch.rand(n, generator=gen) > 0.3).to(torch.uint8)
    k[n - (n % 4):] = 1
    if n >= 4:
        k[0] = 0
    return k


def cast_ties(shape, dtype, seed=3):
    """Values for cast_input: random, with fp64 values planted that lie just off an fp32 value which is itself an exact tie of the bf16
    rounding (1 + 2^-8 + 2^-40 -> fp32 1 + 2^-8 -> bf16 1.0 by ties-to-even, where one rounding from fp64 gives 1 + 2^-7)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen, dtype=torch.float64) * 3
    flat = x.reshape(-1)
    n = flat.numel()
    pos = torch.randint(0, n, (min(n, 64),), generator=gen)
    k = torch.arange(pos.numel())
    base = torch.where(k % 2 == 0, torch.tensor(1.0 + 2.0 ** -8), torch.tensor(1.0 + 2.0 ** -7 + 2.0 ** -8)).double()
    off = 2.0 ** -40 if dtype == torch.float64 else 0.0
    sign = torch.where(k % 3 == 0, -1.0, 1.0).double()
    flat[pos] = sign * (base + torch.where(k % 2 == 0, off, -off)) * (2.0 ** (k % 7 - 3).double())
    flat[n - 1] = 1.0 + 2.0 ** -8 + off
    return x.to(dtype)
