"""Attention / wide-LayerNorm route matrix (GPU): the fused attention of csrc/flash_attn.hip in all three tilings, the windowed
attention and the wide LayerNorm of csrc/swin.hip, the unfused ViT helpers of csrc/attn_loss_optim.hip and the token mean, each with
a per-element bound.

Each case first asserts WHICH kernels it launched (route_probe.routed), then checks every output element against an fp64
restatement on the same bf16-exact inputs: route_probe.attn_ref (plain fp64 softmax / matmul, as test_gpu_flash.reference),
route_probe.window_ref (oracle/swin_oracle.py window_partition, relative_position_index, shift_mask) and route_probe.ln_wide_ref
(swin_oracle.layer_norm).  Channel-slice views have NaN slack, on inputs (a read of it would poison an output) and on outputs (it
must stay NaN).  A NaN output never passes a bound.  Routes are driven by shapes only, except flash tiling 2 (below).

Bounds: |y - ref| <= c*u*mag + ext + tiny for every element, u = 2^-8 for bf16 outputs and 2^-20 for fp32 ones, c_f32(K) =
4 + sqrt(K)/8 for K-term fp32 sums (route_probe).  mag is the operation on absolute values; ext carries score errors through the
softmax.  The terms, checked against each kernel's arithmetic:
  * score error ds_ik = c_f32(d)*2^-20*(a_ik + max_k a_ik + ln N), a = scale*|q|.|k| + |bias| + |mask|: the fp32 dot product, the
    rounding of the scaled score and of its difference to the running maximum that feeds exp2 / __expf (up to a_ik + max a), and
    the lse subtracted in the recomputing backward (ln N).  A probability then carries the relative error r_ik = ds_ik + sum_j
    P_ij ds_ij + c_f32(N)*2^-20 (its row's softmax and the fp32 normaliser), and ext = the mag formula with P*r in place of P.
  * O: mag = sum_k P|V_k|, c = 4.  out32 (fp32): c = 16 + c_f32(N) - the forward feeds P to the MFMA as hi + lo bf16 terms, whose
    lo rounding is 2^-16 of P at worst (16 units of 2^-20), plus the fp32 sums over N keys.
  * lse (log2 units): bound = (sum_k P ds + c_f32(N)*2^-20)/ln 2 + 2^-20*|lse|.
  * delta = sum dO*O: mag = |dO|.mag(O); with out32 u = 2^-20, c = 16 + c_f32(N) + c_f32(128); without it O's bf16 rounding, c = 4.
  * dS_ik = P_ik(dP_ik - delta_i): mag = P_ik(|dO_i|.|V_k| + |dO_i|.mag(O_i)).  dQ / dK / dV: mag = scale*sum_k mag(dS)|K_k|,
    scale*sum_i mag(dS)|Q_i|, sum_i P|dO_i|.  Flash rounds dS (and P for dV) to bf16 before the last GEMM: c = 8 (that rounding,
    without out32 delta's O rounding, the output's own).  The window kernels keep them fp32 (scalar) or hi + lo (MFMA): c = 4.
  * dtable (fp32): the sum of dS over B*nW*N pairs per bin, c = c_f32(B*nW*N), mag = sum mag(dS), plus |the destination's prior
    value| - reduce_finish ADDS into it (every case pre-fills dtable / dgamma / dbeta with non-zero values).
  * ln_wide: y mag |gamma*xhat| + |beta|; dx mag rstd*(|gamma dy| + mean|gamma dy| + |xhat|*mean|gamma dy xhat|), c = 4; dgamma /
    dbeta: c_f32(M), mag sum|dy*xhat|, sum|dy|.  ext: the fp32 mean's rounding 2^-20|mean| times rstd enters xhat - what a row of
    zero variance (rstd = eps^-1/2) shows.
  * softmax_rows: p32 fp32 c_f32(n), mag p*(1 + |scale*s| + |max|) (the rounding of scale*s and of its difference to the max that
    __expf amplifies); pbf bf16 c = 4 mag p; ds bf16 c = 4 mag scale*p*(|dp| + sum p|dp|).  transpose_batched /
    cast_f32_to_bf16_batched: bitwise.  token_mean: fp32 c_f32(L) mag mean|x|; its backward bf16 c = 4 mag |dy|/L.
Each checked output prints its worst ratio err / bound (run with -s to read them).

Inputs: bf16-exact normals with one rare large element.  Every flash (image, head) has four engineered query rows (channels
120..127 of q are zero elsewhere, so they only score these rows): LATE MAX (row N-1: its max key, N-1, sits in the last key tile
>= 28 nats above the rest - the online rescale), ALL-NEGATIVE (row 1: every real score <= -32, so with N % 64 != 0 an unmasked
padded key of score 0 would take nearly all the weight), ZERO QUERY (row 0: uniform P) and TIE (row N-2: keys 0 and N-1, different
tiles for N > 64, tie for the max).  The key-bias property is checked too: with out32 the column sums of dK over the keys vanish
(to the random-walk sum of dK's bf16 roundings, 8*2^-8*sqrt(sum_k mag^2)).

Routes, and the kernels their cases assert:
  * flash_fwd_kernel / flash_bwd_dq_kernel / flash_bwd_dkv_kernel <1, 4> and <1, 8> (fa_variant: <1, 8> when B*H*ceil(N/128) >=
    256): N in {1, 63, 64, 65, 127, 129, 200, 1000, 1024, 2000}, heads 1-4, with and without out32, qkv / out / dO / dqkv as
    channel-slice views (test_flash_routes); <2, 4> only under USSEG_FLASH_TILE=2, which is read once per process: a child
    process (tests/attn_tile_worker.py) runs cases of the same matrix (test_flash_tiling2).
  * softmax_rows_fwd_kernel / softmax_rows_bwd_kernel at n < 64, n % 64 != 0 and rows % 4 != 0 (test_softmax_rows);
    transpose_batched_kernel and cast_f32_bf16_batched_kernel at R, C not multiples of 32 (test_transpose_batched, test_cast_batched):
    the launches of VisionTransformer.Attention with need_weights=True, driven directly.
  * window_attn_kernel<false|true, 2|4|8>: head sizes 8, 40, 64 (64 at ws 8 needs > 48 KB of dynamic LDS both ways), every shift
    0..ws-1, H = ws for the last shift (test_window_scalar).
  * window_attn_mfma_kernel<*, true> (one window per block) and <*, false> with forward wpb 2 / 4 and backward wpb 2 / 4 / 8 / 16,
    nW = 30 (not a multiple of the starting wpb), with and without shift; the wpb is not in the kernel name, each case states it
    from wa_launch's arithmetic (test_window_mfma).  Large cases check the first and last image; dtable always sums all of them.
  * reduce_finish_kernel (every backward here) and reduce_finish_batched_kernel inside ops.overlap_region (the *_deferred cases).
  * ln_wide_kernel<1|2|4|8, false|true>: C in {8, 512, 520, 1024, 1032, 2048, 2056, 3072, 3080, 4096}, M in {1, 4k+3, 16387} (the
    forward's grid-stride loop runs past 4096*4 rows, the backward's past 512*4; at C >= 2048 512 workgroups * 2C floats exceed
    usseg_reduce_ws_floats() and the grid shrinks; the backward's 16*C bytes of LDS pass 48 KB at C = 4096), distinct
    ldx / ldy / lddy / lddx with NaN slack, rows of zero variance (test_ln_wide).
  * token_mean_fwd_kernel / token_mean_bwd_kernel (test_token_mean).
  * ops-level refusals: flash lse / delta / out32 not dense fp32 of the indexed size, window dqkv without qkv's row stride, refused
    before any launch (test_attention_wrappers_refuse_bad_views).
Routes no shape reaches: the scalar ws = 8 kernel at d = 32 (USSEG_WINATTN_MFMA=0, read once per process and not set here; the
scalar ws = 8 kernel itself runs at d = 8, 40, 64).
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from route_probe import (U_BF16, U_F32, acheck, attn_ref, bf, c_f32, ln_wide_ref, routed, window_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
HERE = os.path.dirname(os.path.abspath(__file__))
TILE = {0: "<1, 4>", 1: "<1, 8>", 2: "<2, 4>"}


def slot(buf_shape, off, width, src=None):
    """A NaN-filled bf16 device buffer and its channel slice [..., off:off+width] (holding src if given)."""
    buf = torch.full(buf_shape, NAN, dtype=torch.bfloat16, device=DEV)
    view = buf[..., off:off + width]
    if src is not None:
        view.copy_(src.to(torch.bfloat16))
    return buf, view


def slack_nan(buf, off, width, what):
    assert torch.isnan(buf[..., :off].float()).all() and torch.isnan(buf[..., off + width:].float()).all(), f"{what}: slack written"


# ------------------------------------------------------------------------------------------------ fused attention
def flash_data(gen, B, N, nh):
    """qkv [B,N,3,nh,128] and dO [B,N,nh,128], bf16-exact fp64, with the engineered rows of the module docstring."""
    f = lambda *s, sc=1.0: torch.randn(*s, generator=gen, dtype=torch.float64) * sc
    x = f(B, N, 3, nh, 128, sc=0.8)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    q[..., 120:] = 0
    k[..., 120:] = 2 * torch.rand(B, N, nh, 8, generator=gen, dtype=torch.float64) - 1
    if N >= 4:
        for row in (0, 1, N - 2, N - 1):
            q[:, row] = 0
        q[:, N - 1, :, 120] = 8.0                  # late max: key N-1, in the last tile
        k[:, N - 1, :, 120] = 8.0
        q[:, 1, :, 121] = 8.0                      # all negative: scale*8*k <= -32 for every key
        k[:, :, :, 121] = -8.0 - 4 * torch.rand(B, N, nh, generator=gen, dtype=torch.float64)
        q[:, N - 2, :, 122] = 8.0                  # tie between keys 0 and N-1
        k[:, 0, :, 122] = 4.0
        k[:, N - 1, :, 122] = 4.0
    v[B - 1, N - 1, nh - 1, 127] = 64.0            # the rare large element, in the last row of the last image and head
    do = f(B, N, nh, 128)
    do[0, N // 2, 0, 5] = -48.0
    return bf(x), bf(do)


def run_flash_case(B, N, nh, o32, view, tiling, seed):
    """One flash case: route, every output bounded, slack untouched, key-bias property.  -> worst ratio per output."""
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(seed)
    hs, scale = 128 * nh, 1.0 / math.sqrt(nh)
    x64, do64 = flash_data(gen, B, N, nh)
    qkv_src, do_src = x64.reshape(B, N, 1, 3 * hs), do64.reshape(B, N, 1, hs)
    if view:
        qbuf, qkv = slot((B, N, 1, 3 * hs + 16), 8, 3 * hs, qkv_src)
        obuf, out = slot((B, N, 1, hs + 24), 16, hs)
        dobuf, d_out = slot((B, N, 1, hs + 24), 16, hs, do_src)
        dqbuf, dqkv = slot((B, N, 1, 3 * hs + 16), 8, 3 * hs)
    else:
        qkv, d_out = qkv_src.to(torch.bfloat16).to(DEV), do_src.to(torch.bfloat16).to(DEV)
        out = torch.full((B, N, 1, hs), NAN, dtype=torch.bfloat16, device=DEV)
        dqkv = torch.full((B, N, 1, 3 * hs), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B * nh, N), NAN, dtype=torch.float32, device=DEV)
    delta = torch.full_like(lse, NAN)
    out32 = torch.full((B, N, hs), NAN, dtype=torch.float32, device=DEV) if o32 else None
    t = TILE[tiling]
    routed(lambda: ops.flash_attn_fwd(qkv, nh, scale, out, lse, out32), f"flash_fwd_kernel{t}")
    routed(lambda: ops.flash_attn_bwd(qkv, nh, scale, out, d_out, lse, delta, dqkv, out32), f"flash_bwd_dq_kernel{t}", f"flash_bwd_dkv_kernel{t}")
    torch.cuda.synchronize()

    heads = lambda t_: t_.to(DEV).permute(0, 2, 1, 3).reshape(B * nh, N, 128)          # [B,N,nh,128] -> [G,N,128]
    back = lambda t_: t_.reshape(B, nh, N, 128).permute(0, 2, 1, 3).reshape(B, N, hs)
    r = attn_ref(heads(x64[:, :, 0]), heads(x64[:, :, 1]), heads(x64[:, :, 2]), heads(do64), scale)
    tag = f"flash{t} B{B} N{N} h{nh}{' o32' if o32 else ''}{' view' if view else ''}"
    res = {}
    res["o"] = acheck(f"{tag} O", out.reshape(B, N, hs), back(r["o"]), back(r["om"]), U_BF16, 4.0, back(r["oext"]))
    res["lse"] = acheck(f"{tag} lse", lse, r["lse"], None, 0, 0, r["lse_b"])
    if o32:
        res["o32"] = acheck(f"{tag} O32", out32, back(r["o"]), back(r["om"]), U_F32, 16 + c_f32(N), back(r["oext"]))
        assert torch.equal(out32.to(torch.bfloat16), out.reshape(B, N, hs)), f"{tag}: out is not bf16(out32)"
        res["delta"] = acheck(f"{tag} delta", delta, r["delta"], r["deltam"], U_F32, 16 + c_f32(N) + c_f32(128), r["deltaext"])
    else:
        res["delta"] = acheck(f"{tag} delta", delta, r["delta"], r["deltam"], U_BF16, 4.0, r["deltaext"])
    dq = dqkv.reshape(B, N, 3 * hs)
    for i, nm in enumerate(("dq", "dk", "dv")):
        res[nm] = acheck(f"{tag} {nm}", dq[..., i * hs:(i + 1) * hs], back(r[nm]), back(r[nm + "m"]), U_BF16, 8.0, back(r[nm + "ext"]))
    if o32:       # rows of dS sum to zero: so do the key gradients over the keys (the key-bias gradient)
        kb = dq[..., hs:2 * hs].double().reshape(B, N, nh, 128).sum(1)
        lim = 8 * U_BF16 * back(r["dkm"]).reshape(B, N, nh, 128).pow(2).sum(1).sqrt() + back(r["dkext"]).reshape(B, N, nh, 128).sum(1)
        res["key_bias"] = acheck(f"{tag} key-bias sum", kb, torch.zeros_like(kb), None, 0, 0, lim)
    if view:
        slack_nan(obuf, 16, hs, "out")
        slack_nan(dqbuf, 8, 3 * hs, "dqkv")
    return res


# (B, N, heads, out32, view, tiling): tiling 1 iff B * heads * ceil(N / 128) >= 256
FLASH = [
    (2, 1, 1, True, False, 0),
    (256, 1, 1, False, True, 1),          # N = 1 with B*H >= 256: seven of eight waves past N
    (3, 63, 2, True, True, 0),
    (2, 64, 3, False, False, 0),
    (64, 65, 4, True, False, 1),          # 8-wave tiling with N < 128: whole waves past N, a one-key ragged tile
    (2, 65, 1, False, True, 0),
    (2, 127, 4, True, True, 0),
    (3, 129, 1, False, False, 0),
    (128, 129, 1, True, True, 1),
    (2, 200, 2, True, False, 0),
    (1, 1000, 3, False, True, 0),
    (8, 1024, 4, True, True, 1),
    (1, 1024, 1, False, False, 0),
    (2, 2000, 2, True, True, 0),
    (16, 2000, 1, False, False, 1),
]


@pytest.mark.parametrize("B,N,nh,o32,view,tiling", FLASH, ids=[f"B{c[0]}_N{c[1]}_h{c[2]}{'_o32' if c[3] else ''}{'_view' if c[4] else ''}" for c in FLASH])
def test_flash_routes(B, N, nh, o32, view, tiling):
    assert (B * nh * ((N + 127) // 128) >= 256) == (tiling == 1)
    run_flash_case(B, N, nh, o32, view, tiling, seed=1000 * nh + N)


# cases the child process runs with USSEG_FLASH_TILE=2 (4 waves x 32 queries / keys)
TILE2 = [(2, 65, 1, True, True), (3, 129, 2, False, False), (1, 1000, 4, True, False), (8, 1024, 4, False, True)]


def test_flash_tiling2(tmp_path):
    """One child process, no retry: a non-zero exit fails the test."""
    out = str(tmp_path / "tile2.json")
    env = dict(os.environ, USSEG_FLASH_TILE="2")
    p = subprocess.run([sys.executable, os.path.join(HERE, "attn_tile_worker.py"), out, json.dumps(TILE2)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    assert p.returncode == 0, f"tiling-2 worker exited {p.returncode}:\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    with open(out) as fh:
        res = json.load(fh)
    assert res["ok"] and len(res["cases"]) == len(TILE2), res


# ------------------------------------------------------------------------------------------------ unfused ViT helpers
@pytest.mark.parametrize("rows,n", [(7, 1), (11, 37), (6, 64), (9, 200), (3, 1000), (5, 2048)])
def test_softmax_rows(rows, n):
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(rows * 7919 + n)
    scale = 0.75
    s = (4 * torch.randn(rows, n, generator=gen, dtype=torch.float64)).float()
    s[rows - 1, n - 1] = 64.0
    s[0] = -40.0 - torch.rand(n, generator=gen).float()                  # an all-negative row
    sd = s.to(DEV)
    pbuf = torch.full((rows * n + 64,), NAN, dtype=torch.float32, device=DEV)
    bbuf = torch.full((rows * n + 64,), NAN, dtype=torch.bfloat16, device=DEV)
    p32, pbf = pbuf[:rows * n].view(rows, n), bbuf[:rows * n].view(rows, n)
    routed(lambda: ops.softmax_rows_fwd(sd, n, scale, p32, pbf), "softmax_rows_fwd_kernel")
    torch.cuda.synchronize()
    x = scale * s.double().to(DEV)
    p = torch.softmax(x, -1)
    mx = x.amax(-1, keepdim=True)
    acheck(f"softmax {rows}x{n} p32", p32, p, p * (1 + x.abs() + mx.abs()), U_F32, c_f32(n))
    acheck(f"softmax {rows}x{n} pbf", pbf, p, p, U_BF16, 4.0)
    # backward on the kernel's own fp32 weights (as Attention.backward feeds it)
    dp = torch.randn(rows, n, generator=gen).to(DEV)
    dsbuf = torch.full((rows * n + 64,), NAN, dtype=torch.bfloat16, device=DEV)
    ds = dsbuf[:rows * n].view(rows, n)
    routed(lambda: ops.softmax_rows_bwd(p32, dp, n, scale, ds), "softmax_rows_bwd_kernel")
    torch.cuda.synchronize()
    P, DP = p32.double(), dp.double()
    want = scale * P * (DP - (P * DP).sum(-1, keepdim=True))
    acheck(f"softmax {rows}x{n} ds", ds, want, scale * P * (DP.abs() + (P * DP.abs()).sum(-1, keepdim=True)), U_BF16, 4.0)
    for buf in (pbuf, bbuf, dsbuf):
        assert torch.isnan(buf[rows * n:].float()).all(), "written past the rows"


@pytest.mark.parametrize("nb1,nb2,R,C,lds", [(2, 3, 45, 70, 80), (1, 4, 33, 31, 40), (3, 1, 1, 97, 104)])
def test_transpose_batched(nb1, nb2, R, C, lds):
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(R * C)
    ss2 = R * lds + 16
    ss1 = nb2 * ss2 + 8
    src = torch.randn(nb1 * ss1 + 64, generator=gen).to(torch.bfloat16).to(DEV)
    dbuf = torch.full((nb1 * nb2 * R * C + 64,), NAN, dtype=torch.bfloat16, device=DEV)
    routed(lambda: ops.transpose_batched(src, R, C, lds, nb1, nb2, (ss1, ss2), dbuf), "transpose_batched_kernel")
    torch.cuda.synchronize()
    want = torch.stack([src[b1 * ss1 + b2 * ss2:b1 * ss1 + b2 * ss2 + R * lds].view(R, lds)[:, :C].T for b1 in range(nb1) for b2 in range(nb2)])
    assert torch.equal(dbuf[:nb1 * nb2 * R * C].view(nb1 * nb2, C, R), want)
    assert torch.isnan(dbuf[nb1 * nb2 * R * C:].float()).all(), "written past the end"


@pytest.mark.parametrize("nb1,nb2,R,C,ldd", [(2, 3, 45, 70, 72), (1, 2, 33, 31, 48)])
def test_cast_batched(nb1, nb2, R, C, ldd):
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(R + C)
    src = (torch.randn(nb1 * nb2, R, C, generator=gen) * 3).to(DEV)
    ds2 = R * ldd + 8
    ds1 = nb2 * ds2 + 16
    dbuf = torch.full((nb1 * ds1 + 64,), NAN, dtype=torch.bfloat16, device=DEV)
    routed(lambda: ops.cast_f32_to_bf16_batched(src, R, C, nb1, nb2, dbuf, ldd, (ds1, ds2)), "cast_f32_bf16_batched_kernel")
    torch.cuda.synchronize()
    hit = torch.zeros(dbuf.numel(), dtype=torch.bool, device=DEV)
    for b1 in range(nb1):
        for b2 in range(nb2):
            o = b1 * ds1 + b2 * ds2
            blk = dbuf[o:o + R * ldd].view(R, ldd)
            assert torch.equal(blk[:, :C], src[b1 * nb2 + b2].to(torch.bfloat16)), (b1, b2)
            hit[o:o + R * ldd].view(R, ldd)[:, :C] = True
    assert torch.isnan(dbuf[~hit].float()).all(), "written outside the destination rows"


# ------------------------------------------------------------------------------------------------ windowed attention
def window_case(gen, B, H, W, heads, d, ws, shift, expect_fwd, expect_bwd, view, deferred=False, keep=None):
    from ultrasound_modeling_amd import ops
    C = heads * d
    f = lambda *s, sc=1.0: bf(torch.randn(*s, generator=gen, dtype=torch.float64) * sc)
    qkv = f(B, H, W, 3 * C)
    qkv[B - 1, H - 1, W - 1, 3 * C - 1] = 16.0        # a large v element at the tail
    qkv[0, H // 2, 0, 0] = -8.0                       # and a large q element
    dout = f(B, H, W, C)
    table = (0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=gen, dtype=torch.float64)).float().double()
    t0 = torch.randn_like(table).float().double()     # the destination's prior value: the finish adds to it
    if view:
        qbuf, qd = slot((B, H, W, 3 * C + 16), 8, 3 * C, qkv)
        dobuf, dod = slot((B, H, W, C + 8), 8, C, dout)
        obuf, od = slot((B, H, W, C + 24), 16, C)
        dqbuf, dqd = slot((B, H, W, 3 * C + 16), 8, 3 * C)
    else:
        qd, dod = qkv.to(torch.bfloat16).to(DEV), dout.to(torch.bfloat16).to(DEV)
        od = torch.full((B, H, W, C), NAN, dtype=torch.bfloat16, device=DEV)
        dqd = torch.full_like(qd, NAN)
    td = table.float().to(DEV)
    dtab = t0.float().to(DEV)
    routed(lambda: ops.window_attn_fwd(qd, td, heads, ws, shift, od), expect_fwd)

    def bwd():
        if deferred:
            with ops.overlap_region():
                return ops.window_attn_bwd(qd, dod, td, heads, ws, shift, dqd, dtab)
        return ops.window_attn_bwd(qd, dod, td, heads, ws, shift, dqd, dtab)
    _, got = routed(bwd, expect_bwd, "reduce_finish_batched_kernel" if deferred else "reduce_finish_kernel")
    if deferred:
        assert "reduce_finish_kernel" not in got, got
    torch.cuda.synchronize()
    keep = list(range(B)) if keep is None else keep
    r = window_ref(qkv.to(DEV), dout.to(DEV), table.to(DEV), heads, ws, shift, keep)
    tag = f"win ws{ws} s{shift} d{d} h{heads} {B}x{H}x{W}"
    acheck(f"{tag} O", od[keep], r["o"], r["om"], U_BF16, 4.0, r["oext"])
    acheck(f"{tag} dqkv", dqd[keep], r["dqkv"], r["dqkvm"], U_BF16, 4.0, r["dqkvext"])
    nW = (H // ws) * (W // ws)
    acheck(f"{tag} dtable", dtab, t0.to(DEV) + r["dtable"], r["dtablem"] + t0.abs().to(DEV), U_F32, c_f32(B * nW * ws * ws), r["dtableext"])
    if view:
        slack_nan(obuf, 16, C, "out")
        slack_nan(dqbuf, 8, 3 * C, "dqkv")


def _scalar_cases():
    out = []
    for ws in (2, 4, 8):
        for sh in range(ws):
            d = (8, 40, 64)[(sh + ws) % 3]
            out.append((ws, sh, d, 1 + sh % 2, ws if sh == ws - 1 else 2 * ws, 3 * ws, sh % 2 == 1, ws == 4 and sh == 2))
    return out


WIN_SCALAR = _scalar_cases()


@pytest.mark.parametrize("ws,shift,d,heads,H,W,view,deferred", WIN_SCALAR,
                         ids=[f"ws{c[0]}_s{c[1]}_d{c[2]}{'_view' if c[6] else ''}{'_deferred' if c[7] else ''}" for c in WIN_SCALAR])
def test_window_scalar(ws, shift, d, heads, H, W, view, deferred):
    gen = torch.Generator().manual_seed(ws * 100 + shift * 10 + d)
    window_case(gen, 2, H, W, heads, d, ws, shift, f"window_attn_kernel<false, {ws}>", f"window_attn_kernel<true, {ws}>", view, deferred)


# (id, B, H, W, heads, shift, forward wpb, backward wpb) at d = 32, C = 512.  wa_launch: wpb starts at 4 (forward) / 16 (backward)
# and halves while nW % wpb != 0 or (nW / wpb) * heads * B < 8192 (forward) / 1024 (backward).
WIN_MFMA = [
    ("one", 2, 16, 24, 2, 3, 1, 1),               # nW 6: 3*2*2 = 12 blocks of two windows - one window per block both ways
    ("bwd2", 2, 64, 64, 16, 0, 1, 2),             # nW 64, B*heads 32: backward 32*32 = 1024 blocks of 2
    ("bwd4", 4, 64, 64, 16, 5, 1, 4),             # B*heads 64: 16*64 = 1024 blocks of 4
    ("bwd8", 8, 64, 64, 16, 0, 1, 8),             # B*heads 128: 8*128 = 1024 blocks of 8
    ("bwd16_fwd2", 16, 64, 64, 16, 3, 2, 16),     # B*heads 256: backward 4*256 = 1024 of 16, forward 32*256 = 8192 of 2
    ("fwd4", 32, 64, 64, 16, 7, 4, 16),           # B*heads 512: forward 16*512 = 8192 blocks of 4
    ("nw30", 8, 40, 48, 16, 2, 1, 2),             # nW 30: 16, 8, 4 do not divide it - backward 15*128 = 1920 blocks of 2
]


def wpb_of(nW, BH, bwd):
    wpb, floor = (16, 1024) if bwd else (4, 8192)
    while wpb > 1 and (nW % wpb != 0 or (nW // wpb) * BH < floor):
        wpb >>= 1
    return wpb


WIN_MFMA += [(c[0] + "_deferred",) + c[1:] for c in WIN_MFMA if c[0] in ("one", "bwd4")]


@pytest.mark.parametrize("B,H,W,heads,shift,fw,bw", [c[1:] for c in WIN_MFMA], ids=[c[0] for c in WIN_MFMA])
def test_window_mfma(request, B, H, W, heads, shift, fw, bw):
    deferred = request.node.callspec.id.endswith("_deferred")
    nW = (H // 8) * (W // 8)
    assert (wpb_of(nW, B * heads, False), wpb_of(nW, B * heads, True)) == (fw, bw)
    gen = torch.Generator().manual_seed(B * 1000 + nW + shift)
    name = lambda bwd, w: f"window_attn_mfma_kernel<{'true' if bwd else 'false'}, {'true' if w == 1 else 'false'}>"
    window_case(gen, B, H, W, heads, 32, 8, shift, name(False, fw), name(True, bw), view=B % 4 == 0, deferred=deferred,
                keep=None if B <= 4 else [0, B - 1])


# ------------------------------------------------------------------------------------------------ wide LayerNorm
def ln_nk(C):
    ch = (C // 8 + 63) // 64
    return 1 if ch <= 1 else (2 if ch <= 2 else (4 if ch <= 4 else 8))


LN_C = [8, 512, 520, 1024, 1032, 2048, 2056, 3072, 3080, 4096]
LN_CASES = [(C, 1, False, False) for C in LN_C] + [(C, 4 * (i + 5) + 3, i % 2 == 0, i == 3) for i, C in enumerate(LN_C)] + \
           [(520, 16387, True, False), (1032, 9000, False, True), (2048, 16387, False, False), (3080, 16387, True, False), (4096, 16387, True, False)]


@pytest.mark.parametrize("C,M,view,deferred", LN_CASES, ids=[f"C{c[0]}_M{c[1]}{'_view' if c[2] else ''}{'_deferred' if c[3] else ''}" for c in LN_CASES])
def test_ln_wide(C, M, view, deferred):
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(C * 31 + M)
    x = bf(torch.randn(M, C, generator=gen, dtype=torch.float64) * 1.3 + 0.2)
    dy = bf(torch.randn(M, C, generator=gen, dtype=torch.float64))
    if M >= 3:
        x[1] = 0.75                   # zero-variance rows
        x[2] = 0.0
        x[M - 1, C - 1] = 40.0        # the rare large element at the tail
    gam = (1 + 0.2 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    bet = (0.1 * torch.randn(C, generator=gen, dtype=torch.float64)).float().double()
    g0, b0 = (torch.randn(C, generator=gen, dtype=torch.float64).float().double() for _ in range(2))
    shape = (1, 1, M, C)
    if view:
        xbuf, xd = slot((1, 1, M, C + 16), 8, C, x.reshape(shape))
        dybuf, dyd = slot((1, 1, M, C + 32), 24, C, dy.reshape(shape))
        ybuf, yd = slot((1, 1, M, C + 24), 16, C)
        dxbuf, dxd = slot((1, 1, M, C + 8), 8, C)
    else:
        xd, dyd = x.reshape(shape).to(torch.bfloat16).to(DEV), dy.reshape(shape).to(torch.bfloat16).to(DEV)
        yd, dxd = torch.full_like(xd, NAN), torch.full_like(xd, NAN)
    gd, bd = gam.float().to(DEV), bet.float().to(DEV)
    dga, dbe = g0.float().to(DEV), b0.float().to(DEV)
    nk = ln_nk(C)
    routed(lambda: ops.ln_wide_fwd(xd, gd, bd, 1e-5, yd), f"ln_wide_kernel<{nk}, false>")

    def bwd():
        if deferred:
            with ops.overlap_region():
                return ops.ln_wide_bwd(xd, dyd, gd, 1e-5, dxd, dga, dbe)
        return ops.ln_wide_bwd(xd, dyd, gd, 1e-5, dxd, dga, dbe)
    _, got = routed(bwd, f"ln_wide_kernel<{nk}, true>", "reduce_finish_batched_kernel" if deferred else "reduce_finish_kernel")
    if deferred:
        assert "reduce_finish_kernel" not in got, got
    torch.cuda.synchronize()
    r = ln_wide_ref(x.to(DEV), dy.to(DEV), gam.to(DEV), bet.to(DEV))
    tag = f"ln_wide C{C} M{M}"
    acheck(f"{tag} y", yd.reshape(M, C), r["y"], r["ymag"], U_BF16, 4.0, r["yext"])
    acheck(f"{tag} dx", dxd.reshape(M, C), r["dx"], r["dxmag"], U_BF16, 4.0)
    dev = lambda t: t.to(DEV)
    acheck(f"{tag} dgamma", dga, dev(g0) + r["dgamma"], r["dgmag"] + dev(g0).abs(), U_F32, c_f32(M), r["dgext"])
    acheck(f"{tag} dbeta", dbe, dev(b0) + r["dbeta"], r["dbmag"] + dev(b0).abs(), U_F32, c_f32(M))
    if view:
        slack_nan(ybuf, 16, C, "y")
        slack_nan(dxbuf, 8, C, "dx")


# ------------------------------------------------------------------------------------------------ token mean
def test_token_mean():
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(5)
    B, H, W, C = 3, 7, 9, 200
    x = bf(torch.randn(B, H, W, C, generator=gen, dtype=torch.float64))
    x[B - 1, H - 1, W - 1, C - 1] = 64.0
    xbuf, xd = slot((B, H, W, C + 16), 8, C, x)
    m, _ = routed(lambda: ops.token_mean_fwd(xd), "token_mean_fwd_kernel")
    L = H * W
    acheck("token_mean", m, x.mean((1, 2)).to(DEV), x.abs().mean((1, 2)).to(DEV), U_F32, c_f32(L))
    dy = torch.randn(B, C, generator=gen).to(DEV)
    dx, _ = routed(lambda: ops.token_mean_bwd(dy, xd), "token_mean_bwd_kernel")
    torch.cuda.synchronize()
    want = (dy.double() / L)[:, None, None, :].expand(B, H, W, C)
    acheck("token_mean dx", dx, want, want.abs(), U_BF16, 4.0)
    slack_nan(xbuf, 8, C, "x")


# ------------------------------------------------------------------------------------------------ wrapper checks
def no_launch(fn):
    """fn() must be refused (AssertionError) before anything is launched on the device."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        with pytest.raises(AssertionError):
            fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU and not e.name.lower().startswith(("memcpy", "memset"))]
    assert not names, names


def test_attention_wrappers_refuse_bad_views():
    from ultrasound_modeling_amd import ops
    B, N, nh = 2, 40, 2
    hs = 128 * nh
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)
    qkv, out, d_out, dqkv = z(B, N, 1, 3 * hs), z(B, N, 1, hs), z(B, N, 1, hs), z(B, N, 1, 3 * hs)
    lse, delta, o32 = z(B * nh, N, dt=torch.float32), z(B * nh, N, dt=torch.float32), z(B, N, hs, dt=torch.float32)
    bad_lse = z(N, B * nh, dt=torch.float32).T                  # the right shape, transposed strides
    short_lse = z(B * nh, N - 1, dt=torch.float32)
    bf_o32 = z(B, N, hs)
    f64_delta = z(B * nh, N, dt=torch.float64)
    wide_o32 = z(B, N, hs + 8, dt=torch.float32)[..., :hs]
    no_launch(lambda: ops.flash_attn_fwd(qkv, nh, 1.0, out, bad_lse, o32))
    no_launch(lambda: ops.flash_attn_fwd(qkv, nh, 1.0, out, short_lse))
    no_launch(lambda: ops.flash_attn_fwd(qkv, nh, 1.0, out, lse, bf_o32))
    no_launch(lambda: ops.flash_attn_bwd(qkv, nh, 1.0, out, d_out, lse, f64_delta, dqkv, o32))
    no_launch(lambda: ops.flash_attn_bwd(qkv, nh, 1.0, out, d_out, lse, delta, dqkv, wide_o32))
    no_launch(lambda: ops.flash_attn_bwd(qkv, nh, 1.0, out, d_out, bad_lse, delta, dqkv, o32))
    # window attention: qkv a channel slice of a wider buffer, dqkv dense - the kernel would write it with qkv's row stride
    Bw, Hw, Ww, C, heads = 1, 8, 8, 64, 2
    qv = z(Bw, Hw, Ww, 3 * C + 16)[..., 8:8 + 3 * C]
    dctx, dense = z(Bw, Hw, Ww, C), z(Bw, Hw, Ww, 3 * C)
    table = z(49, heads, dt=torch.float32)
    dtable = torch.zeros_like(table)
    no_launch(lambda: ops.window_attn_bwd(qv, dctx, table, heads, 4, 0, dense, dtable))
