"""fp64 restatement of the fused tile kernels (csrc/cardinal.hip, csrc/stem.hip), one function per STAGE, for test_gpu_fused_routes.py
and test_cpu_fused_restatement.py.  Every function takes fp64 NHWC tensors (on the CPU or on the device) and the PACKED operands the
kernels read, and returns the exact result and its magnitude (the same operation on absolute values).  A test applies a stage to the
bf16-exact tensor the kernel itself stored in front of it, so each bound covers one operation and one rounding.

Packed operands (layers.Conv2D.pack_jobs): forward wp_f[co, t*cin_p + ci] = w[ky, kx, ci, co], backward-data wp_d[ci, t*cout_p + co] =
w[ky, kx, ci, co], tap t = 3*ky + kx of the Keras kernel (cross-correlation, zero padding).

Launcher arithmetic restated here (csrc/cardinal.hip CardBwdCfg / LnbCfg / launch_bwd, csrc/stem.hip usseg_conv3_dgrad_actbwd):
card_bwd_lds, card_bwd_grid, dgrad_grid, walk.
"""
import torch
import torch.nn.functional as F

from route_probe import U_BF16, act_d, bf, norm_ref, seam_data

ALPHA = 0.3
P = 3
CONFIGS = [(32, 3, 10, 64), (64, 7, 21, 128), (128, 14, 42, 256), (256, 28, 85, 512)]
REDUCE_MAX_BLOCKS = 1024      # common.h USSEG_REDUCE_MAX_BLOCKS


def r8(n):
    return (n + 7) // 8 * 8


def r16(n):
    return (n + 15) // 16 * 16


def dims(cfg):
    cin, cv11, cvkk, oc = cfg
    U, V = P * cv11, P * cvkk
    return U, V, r8(U), r8(V)


# ------------------------------------------------------------------------------------------------ packed operands
def pack_f(w, cin_p=None, rows=None):
    """w [k,k,Ci,Co] -> the forward operand [rows, k*k*cin_p] (bf16-exact values stay exact)."""
    k, _, ci, co = w.shape
    cin_p, rows = cin_p or r8(ci), rows or r16(r8(co))
    out = torch.zeros(rows, k * k, cin_p, dtype=w.dtype)
    out[:co, :, :ci] = w.reshape(k * k, ci, co).permute(2, 0, 1)
    return out.reshape(rows, k * k * cin_p)


def pack_d(w, cout_p=None, rows=None):
    """w [k,k,Ci,Co] -> the backward-data operand [rows, k*k*cout_p]."""
    k, _, ci, co = w.shape
    cout_p, rows = cout_p or r8(co), rows or r16(r8(ci))
    out = torch.zeros(rows, k * k, cout_p, dtype=w.dtype)
    out[:ci, :, :co] = w.reshape(k * k, ci, co).permute(1, 0, 2)
    return out.reshape(rows, k * k * cout_p)


def block_diagonal(paths):
    """[P][3,3,ci,co] per-path kernels -> the grouped conv as one dense kernel [3,3,P*ci,P*co] (zero off the diagonal)."""
    k, _, ci, co = paths[0].shape
    w = torch.zeros(k, k, len(paths) * ci, len(paths) * co, dtype=paths[0].dtype)
    for p, blk in enumerate(paths):
        w[:, :, p * ci:(p + 1) * ci, p * co:(p + 1) * co] = blk
    return w


def _taps(x, wt, sign):
    """x [B,H,W,Ci], wt [T,Ci,Co], T = 1 or 9: y[p] = sum_t x[p + sign*(ky - 1, kx - 1)] @ wt[t] with zero padding."""
    B, H, W, _ = x.shape
    if wt.shape[0] == 1:
        return x @ wt[0]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = None
    for t in range(9):
        oy, ox = sign * (t // 3 - 1), sign * (t % 3 - 1)
        term = xp[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W] @ wt[t]
        y = term if y is None else y + term
    return y


def conv_fwd(x, wp, bias, T, cout):
    """The forward conv of packed operand wp [rows, T*cp] on x [B,H,W,cp] (+ bias [>= cout]) -> (y [B,H,W,cout], mag)."""
    cp = x.shape[-1]
    wt = wp.double().to(x.device).reshape(wp.shape[0], T, cp)[:cout].permute(1, 2, 0)
    b = bias.double().to(x.device)[:cout]
    return _taps(x, wt, 1) + b, _taps(x.abs(), wt.abs(), 1) + b.abs()


def conv_dgrad(dy, wd, cin):
    """The 3x3 backward-data pass of packed operand wd [rows, 9*cp] on dy [B,H,W,cp] -> (dx [B,H,W,cin], mag):
    dx[p, ci] = sum_t dy[p - (ky - 1, kx - 1), co] * wd[ci, t, co]."""
    cp = dy.shape[-1]
    wt = wd.double().to(dy.device).reshape(wd.shape[0], 9, cp)[:cin].permute(1, 2, 0)
    return _taps(dy, wt, -1), _taps(dy.abs(), wt.abs(), -1)


def lrelu(v):
    return torch.where(v >= 0, v, ALPHA * v)


def _slope(cond):
    """1 where cond, else alpha, in fp64 (torch.where on two Python scalars would give fp32)."""
    return cond.double() + ALPHA * (~cond).double()


# ------------------------------------------------------------------------------------------------ cardinal stages
def ln_lrelu(x, gamma, beta, G, dy=None):
    """Per-pixel LayerNorm over G groups + LeakyReLU of x [B,H,W,C] (route_probe.norm_ref: y, ymag, and with dy the backward)."""
    C = x.shape[-1]
    return norm_ref(x.reshape(-1, C), gamma.to(x.device), beta.to(x.device), "lrelu", G, dy=None if dy is None else dy.reshape(-1, C))


def tile_sums(y, tile=8):
    """[B,H,W,C] -> the sums over each tile x tile block's in-image pixels [B, tiles, C], tiles row-major, and the sums of |y|."""
    B, H, W, C = y.shape
    th, tw = -(-H // tile), -(-W // tile)
    yp = F.pad(y, (0, 0, 0, tw * tile - W, 0, th * tile - H)).reshape(B, th, tile, tw, tile, C)
    return yp.sum((2, 4)).reshape(B, th * tw, C), yp.abs().sum((2, 4)).reshape(B, th * tw, C)


def fuse_bwd(v_raw, dout, g2, be2, sa_s, sa_dg, mult):
    """conv2_bn's backward with the split-attention re-weighting's backward folded in (dy_eff = mult*s[b]*dout + dg[b]): norm_ref's
    result with the FUSE magnitudes (test_gpu_norm_routes.py: g built from |dout|*|mult*s| + |dg|)."""
    B, H, W, V = v_raw.shape
    se = sa_s.to(v_raw.device).repeat_interleave(H * W, 0)
    ge = sa_dg.to(v_raw.device).repeat_interleave(H * W, 0)
    do = dout.reshape(-1, V)
    r = ln_lrelu(v_raw, g2, be2, P, dy=mult * se * do + ge)
    m = ln_lrelu(v_raw, g2, be2, P, dy=mult * se.abs() * do.abs() + ge.abs())
    for k in ("dxmag", "dxext", "dgmag", "dbmag", "dgext", "dbext"):
        r[k] = m[k]
    r["kink"] = r["kink"] | m["kink"]
    return r


def conv1_bwd(u_raw, dv, w2d, g1, be1):
    """dcat[..., :U] and the three conv1-side sums from the STORED dv [B,H,W,Vp]: du64 = the fp64 backward-data pass of dv, then the
    LayerNorm backward of (u_raw, du64).  The kernel rounds du to bf16 in LDS: |du - du64| <= e = 4*2^-8*mag(du) per element, and the
    LayerNorm backward is linear in its dy, so that error reaches dx as at most
        rstd*(|gamma|*a*e + mean(|gamma|*a*e) + |xhat|*mean(|gamma|*a*e*|xhat|))      (means over the group, a = |act'|, 1 at a kink element)
    and the sums as sum a*e*|xhat| (dgamma), sum a*e (dbeta) and the sum of the dx term (dbias): the keys du_dx, du_dg, du_db, du_dbias."""
    B, H, W, U = u_raw.shape
    M, cg = B * H * W, U // P
    du, dumag = conv_dgrad(dv, w2d, U)
    r = ln_lrelu(u_raw, g1, be1, P, dy=du)
    e = 4.0 * U_BF16 * dumag.reshape(M, U)
    a = torch.where(r["kink"], torch.ones_like(e), act_d(r["pre"], "lrelu").abs())
    xa = r["xh"].abs()
    red = lambda t: t.view(M, P, cg).mean(-1, keepdim=True).expand(M, P, cg).reshape(M, U)
    gae = g1.to(e.device).abs() * a * e
    r["du_dx"] = r["rstd"] * (gae + red(gae) + xa * red(gae * xa))
    r["du_dg"], r["du_db"], r["du_dbias"] = (a * e * xa).sum(0), (a * e).sum(0), r["du_dx"].sum(0)
    r["du"], r["dumag"] = du, dumag
    return r


# ------------------------------------------------------------------------------------------------ stem stages
def bn_lrelu_pool(c2, gamma, beta, mean, var, eps):
    """Inference BatchNorm + LeakyReLU + 2x2 mean of c2 [B,H,W,C] -> (pooled [B,H/2,W/2,C], mag)."""
    B, H, W, C = c2.shape
    g, b, mu, rstd = (t.double().to(c2.device) for t in (gamma, beta, mean, (var.double() + eps).rsqrt()))
    xh = (c2 - mu) * rstd
    pool = lambda t: t.reshape(B, H // 2, 2, W // 2, 2, C).mean((2, 4))
    return pool(lrelu(g * xh + b)), pool((g * xh).abs() + b.abs())


def dgrad_actbwd(dy, wd, yact, mode, gamma=None, beta=None, var=None, eps=1e-3):
    """usseg_conv3_dgrad_actbwd: d = the backward-data pass of dy (kept in fp32 by the kernel), then from the stored ACTIVATED tensor yact
    mode 2: dh = d*(yact > 0 ? 1 : alpha), dx = dh*gamma*rstd, xhat = (act^-1(yact) - beta)/gamma, sums dgamma = sum dh*xhat, dbeta = sum dh,
            dbias = sum dx (fp32 values);
    mode 0: dx = d*(yact >= 0 ? 1 : alpha); dbias is the column sum of the STORED bf16 dx (stem.hip: 'the sums are those of the STORED
            (bf16) values', as usseg_act_bwd_colsum), which the caller forms from the kernel's dx."""
    co = yact.shape[-1]
    d, dm = conv_dgrad(dy, wd, co)
    if mode == 0:
        s = _slope(yact >= 0)
        return dict(dx=d * s, dxmag=dm * s)
    g, b, rstd = (t.double().to(dy.device) for t in (gamma, beta, (var.double() + eps).rsqrt()))
    s = _slope(yact > 0)
    dh, dhm = d * s, dm * s
    xh = (torch.where(yact >= 0, yact, yact / ALPHA) - b) / g
    red = lambda t: t.sum((0, 1, 2))
    return dict(dx=dh * g * rstd, dxmag=dhm * (g * rstd).abs(), dgamma=red(dh * xh), dgmag=red(dhm * xh.abs()), dbeta=red(dh), dbmag=red(dhm),
                dbias=red(dh * g * rstd), dbimag=red(dhm * (g * rstd).abs()))


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
def vec(gen, n, base=1.0, sc=0.2, neg=False):
    """fp32-exact fp64 per-channel vector; with `neg`, every third entry negated."""
    v = (base + sc * torch.randn(n, generator=gen, dtype=torch.float64)).float().double()
    if neg:
        v[::3] = -v[::3]
    return v


def card_weights(cfg):
    """bf16-exact weights of one channel configuration as packed operands, fp32-exact vectors (gamma of both signs); fp64 on the CPU."""
    cin, cv11, cvkk, oc = cfg
    U, V, Up, Vp = dims(cfg)
    gen = torch.Generator().manual_seed(9000 + cin)
    rn = lambda *s, sc: bf(torch.randn(*s, generator=gen, dtype=torch.float64) * sc)
    w1, wsc = rn(1, 1, cin, U, sc=cin ** -0.5), rn(1, 1, cin, oc, sc=cin ** -0.5)
    w2 = block_diagonal([rn(3, 3, cv11, cvkk, sc=(9 * cv11) ** -0.5) for _ in range(P)])
    p = dict(w1=pack_f(w1, cin, r16(Up)), w2=pack_f(w2, Up, r16(Vp)), w2d=pack_d(w2, Vp, r16(Up)), wsc=pack_f(wsc, cin, oc),
             keras=dict(w1=w1, w2=w2, wsc=wsc))
    for nm, n in (("1", U), ("2", V), ("sc", oc)):
        p["b" + nm], p["g" + nm], p["be" + nm] = vec(gen, n, 0.0, 0.1), vec(gen, n, neg=True), vec(gen, n, 0.0, 0.1)
    return p


def card_bwd_inputs(cfg, B, H, W):
    """The inputs of a cardinal_bwd case (8-pixel seams in both directions), sa_s / sa_dg per image, the nine non-zero initial sums."""
    cin, cv11, cvkk, oc = cfg
    U, V, Up, Vp = dims(cfg)
    gen = torch.Generator().manual_seed(77000 + 1000 * B + 10 * H + W)
    sd = lambda c: seam_data(gen, B, H, W, c, seam=8, cols=True)
    d = dict(v_raw=sd(V), u_raw=sd(U), sc_raw=sd(oc), dout=sd(V), dsc=sd(oc))
    d["sa_s"] = torch.rand(B, V, generator=gen, dtype=torch.float64).float().double()
    d["sa_dg"] = (0.05 * torch.randn(B, V, generator=gen, dtype=torch.float64)).float().double()
    d["init"] = [(0.5 * torch.randn(n, generator=gen)).double() for n in (V, V, V, U, U, U, oc, oc, oc)]
    return d


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def _lnb_lds(cp, ng, fuse):
    cph = cp * 8
    pg = 1 if cph >= 256 else 256 // cph
    return 2 * (64 * (cph + 8) * 2) + 64 * ng * 16 + 4 * 1024 * 4 + pg * 3 * cph * 4 + (2 * cph * 4 if fuse else 0)


def card_bwd_lds(cfg):
    """CardBwdCfg<CV11, CVKK, OC>::LDS_B."""
    cin, cv11, cvkk, oc = cfg
    U, V, Up, Vp = dims(cfg)
    vt_b, ut_b = 100 * (Vp + 8) * 2, 64 * (Up + 8) * 2
    pg = lambda cph: min(32, 256 // (cph // 4))
    red_b = max(pg(Vp) * 3 * Vp, pg(Up) * 3 * Up) * 4
    card = 2 * vt_b + 128 * 3 * 16 + 4 * 1024 * 4 + red_b + 2 * Vp * 4 + 128 + ut_b
    return max(card, _lnb_lds(oc // 8, 1, False))


def card_bwd_grid(cfg, B, H, W, g_env=0):
    """launch_bwd -> (ntiles, sc_tiles, G workgroup pairs)."""
    U, V, Up, Vp = dims(cfg)
    ntiles, sc_tiles = -(-H // 8) * -(-W // 8) * B, -(-B * H * W // 64)
    per_cu = max(1, 160 * 1024 // (2 * card_bwd_lds(cfg)))
    G = g_env if g_env > 0 else 256 * per_cu
    G = min(G, max(ntiles, sc_tiles), REDUCE_MAX_BLOCKS)
    while G > 1 and G * 3 * (Vp + Up + cfg[3]) > REDUCE_MAX_BLOCKS * 3 * 512:
        G >>= 1
    return ntiles, sc_tiles, G


def dgrad_grid(B, H, W):
    """usseg_conv3_dgrad_actbwd -> (ntiles, workgroups)."""
    ntiles = -(-H // 16) * -(-W // 16) * B
    return ntiles, min(ntiles, 512)


def walk(ntiles, G):
    """The grid property of a persistent walk t = blk, blk + G, ...: 'one' tile per workgroup, a ragged 'second' trip, or 'three+' trips."""
    trips = -(-ntiles // G)
    return "one" if trips == 1 else ("second" if trips == 2 else "three+")


# ------------------------------------------------------------------------------------------------ the chains with bf16 storage points
def card_chain(x, prm, cfg, rounded=True):
    """cardinal_fwd as a chain of the stages above; with `rounded`, bf16 at the kernel's storage points (the CPU stand-in for its tensors)."""
    cin, cv11, cvkk, oc = cfg
    U, V, Up, Vp = dims(cfg)
    q = bf if rounded else (lambda t: t)
    shp = x.shape[:3]
    pad = lambda t, n: F.pad(t, (0, n - t.shape[-1]))
    u_raw = q(conv_fwd(x, prm["w1"], prm["b1"], 1, U)[0])
    u = q(ln_lrelu(u_raw, prm["g1"], prm["be1"], P)["y"].reshape(*shp, U))
    v_raw = q(conv_fwd(pad(u, Up), prm["w2"], prm["b2"], 9, V)[0])
    y = q(ln_lrelu(v_raw, prm["g2"], prm["be2"], P)["y"].reshape(*shp, V))
    sc_raw = q(conv_fwd(x, prm["wsc"], prm["bsc"], 1, oc)[0])
    sc = q(ln_lrelu(sc_raw, prm["gsc"], prm["besc"], 1)["y"].reshape(*shp, oc))
    return dict(u_raw=u_raw, u=u, v_raw=v_raw, y=y, sc_raw=sc_raw, sc=sc)


def kink_share(ref):
    """The share of a LayerNorm backward's dx elements inside the kink window."""
    return ref["kink"].sum().item() / ref["kink"].numel()
