"""Test helpers for the conv and norm route matrices: which device kernels a call launched, and a per-element error bound.

kernels(fn) runs fn under torch.profiler (device activity only) and returns (fn's result, the demangled names of the
device kernels it launched, in launch order).  A call that records no device kernel fails the test: a probe that cannot
see the launches must never turn into a pass or a skip.

assert_elementwise(y, ref, mag, u, c) checks |y - ref| <= c * u * mag + tiny for every element, in fp64, where mag is
the same operation applied to |x| and |w| (so it bounds every partial sum the kernel formed).  The relative-L2 checks
of test_gpu_ops.py average an error over the whole tensor; this one fails on a single wrong element.

norm_ref / check_norm_bwd restate the LayerNorm / BatchNorm + activation forward and backward in fp64 with the magnitudes and the
kink rule that test_gpu_norm_routes.py states once in its docstring.

attn_ref / window_ref / ln_wide_ref restate the attention kernels and the wide LayerNorm in fp64 with the magnitudes and the
score-error terms that test_gpu_attn_routes.py states once in its docstring; acheck bounds an output on the device (with `skip`, all
but the kink-excluded elements).  seam_data(..., seam=8, cols=True) places the last image's values next to the row AND column seams of a
2-D tile kernel (test_gpu_fused_routes.py).

small_deferral(floats, first_producer=True) defers the finishing reductions of the current stream into a partial-row region of only
`floats` floats, so that a test can place a launch's regions against the end of a full region.
"""
import contextlib
import math

import pytest
import torch

import usseg_oracle as O

U_BF16 = 2.0 ** -8      # unit roundoff of a bf16 output (one final rounding)
U_F32 = 2.0 ** -20      # fp32 outputs: 2^-24 per rounding, x16 margin; the callers scale c with the sum length K
C_BOUND = 4.0           # stated constant for bf16 outputs (one final rounding of 2^-9 dominates the fp32 sum's error);
                        # fp32 outputs use c = 4 + sqrt(K)/8 - a chosen constant that follows the random-walk growth of a K-term
                        # fp32 sum, not a proven worst case (which grows like K)
TINY = 1e-6
DEV = "cuda"


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def seam_data(gen, B, H, W, C, scale=1.0, seam=16, cols=False):
    """bf16-exact fp64 NHWC data with one large element and a last image that is zero except near the `seam`-row seams (16 by default)
    and in the last two rows; with `cols`, also kept next to the `seam`-column seams and in the last two columns (2-D tile kernels)."""
    x = bf(torch.randn(B, H, W, C, generator=gen, dtype=torch.float64) * scale)
    if B > 1 and H > 4:
        near = lambda n: torch.tensor([r % seam in (0, seam - 1) or r >= n - 2 for r in range(n)])
        keep = near(H)[:, None].expand(H, W)
        if cols:
            keep = keep | near(W)[None, :]
        x[B - 1][~keep] = 0
    x[B - 1, H - 1, W - 1, C - 1] = 64 * scale      # the last element of the tensor: the ragged tail of every walk
    x[0, H // 2, 0, 0] = -48 * scale
    return x


def to_dev(x64, ld=None, off=0, fill=0.0):
    """fp64 NHWC -> device bf16 view [..., off:off+roundup(C,8)] of a buffer with `ld` channels (default: no slack)."""
    B, H, W, C = x64.shape
    cp = (C + 7) // 8 * 8
    ld = ld or cp
    buf = torch.full((B, H, W, ld), fill, dtype=torch.bfloat16)
    buf[..., off:off + C] = x64.to(torch.bfloat16)
    if cp > C:
        buf[..., off + C:off + cp] = 0
    buf = buf.to(DEV)
    return buf, buf[..., off:off + cp]


def nan_view(B, H, W, cp, ld, off):
    """A NaN-filled device bf16 buffer [B,H,W,ld] and its channel-slice view [..., off:off+cp] (an output written through the view)."""
    buf = torch.full((B, H, W, ld), float("nan"), dtype=torch.bfloat16, device=DEV)
    return buf, buf[..., off:off + cp]


def outside_untouched(buf, off, cp, what):
    assert torch.isnan(buf[..., :off].float()).all() and torch.isnan(buf[..., off + cp:].float()).all(), f"{what}: outside the view"


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name for e in evs if not e.name.startswith(("Memcpy", "Memset", "memcpy", "memset"))]
    if not names:
        pytest.fail("the profiler recorded no device kernel for this call: the route cannot be checked")
    return out, names


@contextlib.contextmanager
def small_deferral(floats, first_producer=True):
    """A deferral context (usseg_defer_begin) on the current stream with a partial-row region of `floats` floats and no slab region;
    with `first_producer`, a one-workgroup LayerNorm backward (64 pixels x 8 channels: 24 floats of partial rows) first takes the
    region's first 64 floats.  The queued finishes run when the block ends."""
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    region = torch.empty(floats, dtype=torch.float32, device=DEV)
    if first_producer:
        x, dy = (to_dev(bf(torch.linspace(-2, 2, 512, dtype=torch.float64).reshape(1, 8, 8, 8) * k))[1] for k in (1, -1))
        v = torch.ones(8, device=DEV)
        g = [torch.zeros(8, device=DEV) for _ in range(3)]
    h = torch.cuda.current_stream().cuda_stream
    L.check(L.load().usseg_defer_begin(h, region.data_ptr(), floats, None, 0), "defer_begin")
    try:
        if first_producer:
            ops.norm_act_bwd(x, dy, 8, v, v, torch.empty_like(x), g[0], g[1], 0, 1, EPS, ops.ACT_LRELU, 0.3, dbias=g[2])
        yield
    finally:
        L.check(L.load().usseg_defer_end(h), "defer_end")


def no_launch(fn):
    """fn() must raise before launching anything on the device."""
    from torch.profiler import ProfilerActivity, profile
    from ultrasound_modeling_amd._lib import UssegError
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        with pytest.raises(UssegError):
            fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU and not e.name.lower().startswith(("memcpy", "memset"))]
    assert not names, names


def short(name):
    """'void conv_halo_persist_kernel<2>(HaloMulti, int)' -> 'conv_halo_persist_kernel<2>'."""
    n = name
    if n.startswith("void "):
        n = n[5:]
    depth = 0
    for i, ch in enumerate(n):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return n[:i].strip()
    return n.strip()


def routed(fn, *expected):
    """Run fn, assert every name in `expected` is a launched kernel (exact short name, or a prefix ending in '<' or
    the bare kernel name), and return fn's result and the short names."""
    out, names = kernels(fn)
    got = [short(n.replace("(anonymous namespace)::", "")) for n in names]
    for e in expected:
        if not any(g == e or (e.endswith("<") and g.startswith(e)) or g.split("<")[0] == e for g in got):
            pytest.fail(f"expected kernel {e!r}, launched {got}")
    return out, got


def assert_elementwise(y, ref, mag, u, c=C_BOUND, tiny=TINY, what=""):
    y = y.detach().double().cpu()
    ref = ref.detach().double().cpu()
    mag = mag.detach().double().cpu()
    assert y.shape == ref.shape == mag.shape, (y.shape, ref.shape, mag.shape)
    err = (y - ref).abs()
    lim = c * u * mag + tiny
    bad = ~(err <= lim)          # a NaN output is out of bounds, not silently inside them
    if bad.any():
        idx = bad.nonzero()
        first = tuple(idx[0].tolist())
        ratio = (err / lim).max().item()
        pytest.fail(f"{what}: {int(bad.sum())} of {y.numel()} elements exceed c*u*(|x|*|w|)+tiny "
                    f"(worst ratio {ratio:.2f}); first at {first}: got {y[first].item():.6g}, ref {ref[first].item():.6g}, "
                    f"bound {lim[first].item():.3g}")


# ------------------------------------------------------------------------------------------------ norm restatement (fp64)
EPS = 1e-3
KINK = 2.0 ** -12
KINK_FRAC = 1e-3
ACTS = {"none": (0, 0.0), "lrelu": (1, 0.3), "relu": (2, 0.0), "elu": (3, 1.0)}


def c_f32(k):
    return 4.0 + math.sqrt(k) / 8.0


def act_f(v, act):
    if act == "lrelu":
        return O.leaky_relu(v)
    if act == "relu":
        return torch.relu(v)
    if act == "elu":
        return O.elu(v)
    return v


def act_d(v, act):
    if act == "lrelu":
        return torch.where(v >= 0, 1.0, ACTS["lrelu"][1]).to(v.dtype)
    if act == "relu":
        return (v > 0).to(v.dtype)
    if act == "elu":
        return torch.where(v > 0, torch.ones_like(v), torch.exp(v.clamp(max=0)))
    return torch.ones_like(v)


def kink_gap(act):
    """1 - the slope left of the kink (0: no kink; ELU with alpha 1 has a continuous slope)."""
    return {"lrelu": 1.0 - ACTS["lrelu"][1], "relu": 1.0}.get(act, 0.0)


def check(what, y, ref, mag, u, c, extra=None, skip=None):
    """assert_elementwise over the elements not in `skip`, with `extra` added to the bound; prints the worst ratio."""
    y, ref, mag = (t.detach().double().reshape(-1) for t in (y, ref, mag))
    ref, mag = ref.to(y.device), mag.to(y.device)
    if extra is not None:
        mag = mag + extra.detach().double().reshape(-1).to(y.device) / (c * u)
    if skip is not None:
        keep = ~skip.reshape(-1).to(y.device)
        y, ref, mag = y[keep], ref[keep], mag[keep]
    ratio = ((y - ref).abs() / (c * u * mag + 1e-6)).max().item() if y.numel() else 0.0
    print(f"\n  bound {what}: worst ratio {ratio:.3f}", end="")
    assert_elementwise(y, ref, mag, u, c, what=what)
    return ratio


def norm_ref(x, gamma, beta, act, G=1, mode=0, mean=None, var=None, mask=None, dy=None, eps=EPS):
    """x [M, C] fp64 on the device.  mode 0: LayerNorm over G groups (O.layer_norm); 1: affine BN with mean/var (O.batch_norm,
    inference); 'batch': BN with the batch statistics (O.batch_norm, training).  Returns the references, the magnitudes, the
    kink set and what its elements could add to each bound."""
    M, C = x.shape
    Cg = C // G
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    if mode == 0:
        pre = torch.cat([O.layer_norm(xr[:, g * Cg:(g + 1) * Cg], gr[g * Cg:(g + 1) * Cg], br[g * Cg:(g + 1) * Cg], eps=eps) for g in range(G)], 1)
        xg = x.view(M, G, Cg)
        mu = xg.mean(-1, keepdim=True)
        rstd = (((xg - mu) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
        xh = ((xg - mu) * rstd).view(M, C)
        rstd = rstd.expand(M, G, Cg).reshape(M, C)
    elif mode == 1:
        pre = O.batch_norm(xr, gr, br, mean, var, training=False)
        rstd = (var + O.KERAS["bn_eps"]).rsqrt().expand(M, C)
        xh = (x - mean) * rstd
    else:
        pre, stats = O.batch_norm(xr, gr, br, torch.zeros_like(gamma), torch.ones_like(gamma), training=True)
        mu, vv = x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
        rstd = (vv + O.KERAS["bn_eps"]).rsqrt().expand(M, C)
        xh = (x - mu) * rstd
    mk = mask if mask is not None else torch.ones_like(x)
    y = act_f(pre, act) * mk
    r = dict(y=y.detach(), pre=pre.detach(), xh=xh, rstd=rstd)
    pm = (gamma * xh).abs() + beta.abs()
    r["ymag"] = pm * mk.abs()
    if mode == "batch":
        r["stats"] = stats
    if dy is None:
        return r
    (y * dy).sum().backward()
    r.update(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
    dyeff = dy.abs() * mk.abs()
    g = act_d(r["pre"], act).abs() * dyeff
    gg = (gamma * g).abs()
    kink = (r["pre"].abs() < KINK * pm) & (dyeff != 0) if kink_gap(act) else torch.zeros_like(x, dtype=torch.bool)
    amb = kink_gap(act) * (gamma * dyeff).abs() * kink
    if mode == 0:
        red = lambda t: t.view(M, G, Cg).mean(-1, keepdim=True).expand(M, G, Cg).reshape(M, C)
        dxmag = rstd * (gg + red(gg) + xh.abs() * red(gg * xh.abs()))
        dxext = rstd * (amb + red(amb) + xh.abs() * red(amb * xh.abs()))
    elif mode == "batch":
        dxmag = rstd * (gg + gg.mean(0) + xh.abs() * (gg * xh.abs()).mean(0))
        dxext = rstd * (amb + amb.mean(0) + xh.abs() * (amb * xh.abs()).mean(0))
    else:
        dxmag, dxext = rstd * gg, rstd * amb
    r.update(dxmag=dxmag, dxext=dxext, kink=kink, dgmag=(g * xh).abs().sum(0), dbmag=g.sum(0),
             dgext=(kink_gap(act) * dyeff * xh.abs() * kink).sum(0), dbext=(kink_gap(act) * dyeff * kink).sum(0))
    return r


def check_norm_bwd(what, M, C, ref, dx, dgam, dbet, dbias=None):
    nk = int(ref["kink"].sum())
    print(f"\n  {what}: {nk} of {M * C} dx elements within the kink window", end="")
    assert nk <= KINK_FRAC * M * C, f"{what}: {nk} kink-excluded elements of {M * C}"
    check(f"{what} dx", dx, ref["dx"], ref["dxmag"], U_BF16, 4.0, extra=ref["dxext"], skip=ref["kink"])
    cf = c_f32(M)
    check(f"{what} dgamma", dgam[:C], ref["dgamma"], ref["dgmag"], U_F32, cf, extra=ref["dgext"])
    check(f"{what} dbeta", dbet[:C], ref["dbeta"], ref["dbmag"], U_F32, cf, extra=ref["dbext"])
    if dbias is not None:
        check(f"{what} dbias", dbias[:C], ref["dx"].sum(0), ref["dxmag"].sum(0), U_F32, cf, extra=ref["dxext"].sum(0))


def kname(bwd, mode, ng, fuse=False, pool=False, res=False):
    b = lambda v: "true" if v else "false"
    return f"norm_act_kernel<{b(bwd)}, {mode}, {ng}, {b(fuse)}, {b(pool)}, {b(res)}>"


def ng_of(G):
    return 1 if G == 1 else (3 if G <= 3 else 4)


# ------------------------------------------------------------------------------------------------ split attention (fp64)
def sa_mlp_ref(gin, prm, norm_mode, act, sigmoid, absval=False):
    """The per-(image, path) MLP in fp64: gin [B,P,Cg] -> (h1, xhat, rstd, pre, a, z, s)."""
    w1, b1, ga, be, mm, mv, w2, b2 = prm
    h1 = torch.einsum("bpc,pch->bph", gin, w1) + b1
    if norm_mode == 0:
        pre = O.layer_norm(h1, ga, be)
        mu = h1.mean(-1, keepdim=True)
        rstd = (((h1 - mu) ** 2).mean(-1, keepdim=True) + O.KERAS["ln_eps"]).rsqrt()
        xh = (h1 - mu) * rstd
    else:
        pre = O.batch_norm(h1, ga, be, mm, mv, training=False)
        rstd = (mv + O.KERAS["bn_eps"]).rsqrt().expand_as(h1)
        xh = (h1 - mm) * rstd
    a = act_f(pre, act)
    z = torch.einsum("bph,prhc->bprc", a, w2) + b2
    s = torch.sigmoid(z) if sigmoid else O.softmax_lastaxis(z)
    return h1, xh, rstd, pre, a, z, s


def sa_mags(y, dout, prm, fw, B, HW, P, R, Cg, Hd, mult, norm_mode, act, sigmoid):
    """The split attention restated on absolute values: -> mags of out, dy and the six parameter gradients.  The MLP's inputs are
    fp32 values it computed itself, so its forward mags carry their sensitivity: xhat -> rstd*(mag(h1) + mean or |moving mean|),
    s -> s*(1 + mag(z) + sum s*mag(z)) (softmax; sigmoid: s*(1 + mag(z))), and the backward runs on those."""
    w1, b1, ga, be, mm, mv, w2, b2 = (t.abs() for t in prm)
    h1, xh, rstd, pre, a, z, s = fw
    yv = y.view(B, HW, P, R, Cg).abs()
    do = dout.view(B, HW, P, 1, Cg).abs()
    gin = mult / HW * yv.sum((1, 3))
    h1m = torch.einsum("bpc,pch->bph", gin, w1) + b1
    xhm = rstd * (h1m + (h1m.mean(-1, keepdim=True) if norm_mode == 0 else mm))
    am = ga * xhm + be
    zm = torch.einsum("bph,prhc->bprc", am, w2) + b2
    sm = s * (1 + zm) if sigmoid else s * (1 + zm + (s * zm).sum(-1, keepdim=True))
    outm = mult * (yv * sm.unsqueeze(1)).sum(3).reshape(B, HW, P * Cg)
    ds = mult * (yv * do).sum(1)                                                # [B,P,R,Cg]
    dz = sm * ds if sigmoid else sm * (ds + (sm * ds).sum(-1, keepdim=True))
    da = torch.einsum("prhc,bprc->bph", w2, dz)

    def back(dpre):          # dpre -> (mag of dg [B,P,Cg], mags of dw1, db1, dgamma, dbeta)
        dxh = dpre * ga
        if norm_mode == 0:
            dh = rstd * (dxh + dxh.mean(-1, keepdim=True) + xhm * (dxh * xhm).mean(-1, keepdim=True))
        else:
            dh = dxh * rstd
        return (mult / HW * torch.einsum("pch,bph->bpc", w1, dh),
                (torch.einsum("bpc,bph->pch", gin, dh), dh.sum(0), (dpre * xhm).sum(0), dpre.sum(0)))
    dgm, g4 = back(da * act_d(pre, act).abs())
    # the kink rule: a pre-activation within 2^-12*mag of the kink may take the other slope; what that could change is added
    kink = pre.abs() < KINK * am
    dge, e4 = back(kink_gap(act) * da * kink)
    dym = mult * sm.unsqueeze(1) * do + (dgm + dge).view(B, 1, P, 1, Cg)
    grads = tuple(a + b for a, b in zip(g4, e4)) + (torch.einsum("bph,bprc->prhc", am, dz), dz.sum(0))
    return outm, dym.reshape(B, HW, P * R * Cg), grads


def sa_reference(y, dout, prm, P, R, Cg, Hd, mult, norm_mode, act, sigmoid):
    """Split attention (ResNest.py:171-199 for R == 1 with mult = radix; TBI_ResNest.py:175-207 for R distinct branches) in fp64 on
    the device: y [B,HW,P*R*Cg], dout [B,HW,P*Cg], prm = (w1 [P,Cg,Hd], b1, gamma, beta, moving mean, moving var [P,Hd],
    w2 [P,R,Hd,Cg], b2 [P,R,Cg]).  -> out, dy and the six parameter gradients (autograd) with their mags (the kink rule's
    ambiguity of the MLP's pre-activations included)."""
    B, HW = y.shape[:2]
    leaves = [y.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in prm]
    yl, w1, b1, ga, be, mm, mv, w2, b2 = leaves
    gin = mult / HW * yl.view(B, HW, P, R, Cg).sum((1, 3))
    fw = sa_mlp_ref(gin, (w1, b1, ga, be, mm.detach(), mv.detach(), w2, b2), norm_mode, act, sigmoid)
    out = mult * (yl.view(B, HW, P, R, Cg) * fw[-1].unsqueeze(1)).sum(3).reshape(B, HW, P * Cg)
    (out * dout).sum().backward()
    fwd = tuple(t.detach() for t in fw)
    outm, dym, gm = sa_mags(y, dout, prm, fwd, B, HW, P, R, Cg, Hd, mult, norm_mode, act, sigmoid)
    return dict(out=out.detach(), outm=outm, dy=yl.grad, dym=dym, grads=(w1.grad, b1.grad, ga.grad, be.grad, w2.grad, b2.grad), gmags=gm)


# ------------------------------------------------------------------------------------------------ attention restatement (fp64)
def acheck(what, y, ref, mag, u, c, extra=None, tiny=TINY, skip=None):
    """|y - ref| <= c*u*mag + extra + tiny for every element (not in the boolean `skip`), evaluated on y's device (NaN fails); prints
    and returns the worst ratio err / bound.  mag may be None (the bound is extra alone)."""
    y = y.detach().double()
    ref = ref.detach().double().to(y.device)
    lim = torch.full_like(ref, tiny)
    if mag is not None:
        lim = lim + c * u * mag.detach().double().to(y.device)
    if extra is not None:
        lim = lim + extra.detach().double().to(y.device)
    assert y.shape == ref.shape == lim.shape, (what, y.shape, ref.shape, lim.shape)
    err = (y - ref).abs()
    bad = ~(err <= lim)
    ratios = (err / lim).nan_to_num(nan=float("inf"))
    if skip is not None:
        keep = ~skip.to(y.device).reshape(y.shape)
        bad, ratios = bad & keep, ratios * keep
    ratio = ratios.max().item() if y.numel() else 0.0
    print(f"\n  bound {what}: worst ratio {ratio:.3f}", end="")
    if bad.any():
        first = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"{what}: {int(bad.sum())} of {y.numel()} elements out of bounds (worst ratio {ratio:.2f}); first at {first}: "
                    f"got {y[first].item():.6g}, ref {ref[first].item():.6g}, bound {lim[first].item():.3g}")
    return ratio


def attn_ref(q, k, v, do, scale, bias=None, bias_abs=None, chunk=1 << 26):
    """Attention restated in fp64 for G independent problems: q, k, v, do [G, N, d] on the device, bias [G, N, N] (or None) added to
    the scaled score s = scale*q.k.  Returns the exact results (o, lse in log2 units, delta = sum_j P*dP, dS = dL/ds = P*(dP - delta),
    dq = scale*dS.k, dk = scale*dS^T.q, dv = P^T.do) and their magnitudes:
      a      = scale*|q|.|k| + |bias|                 (what the fp32 score is summed from)
      ds     = c_f32(d)*2^-20*(a + max_row a + ln N)  (score error: the fp32 dot product and the rounding of s - running max)
      r      = ds + sum_j P*ds + c_f32(N)*2^-20      (relative error of a probability: its score, the row's softmax, the normaliser)
      om     = P.|v|                                  (oext = (P*r).|v|)
      dsm    = P*(|do|.|v|^T + |do|.om)                (dsext = dsm*r)
      dqm    = scale*dsm.|k|,  dkm = scale*dsm^T.|q|,  dvm = P^T.|do|   (and the ext terms the same way from dsext, P*r)
      lse_b  = (sum_j P*ds + c_f32(N)*2^-20)/ln 2 + 2^-20*|lse|   (an absolute bound)"""
    G, N, d = q.shape
    per = max(1, chunk // (N * N))
    outs = []
    for g0 in range(0, G, per):
        sl = slice(g0, min(G, g0 + per))
        outs.append(_attn_ref_chunk(q[sl], k[sl], v[sl], do[sl], scale, None if bias is None else bias[sl],
                                    None if bias_abs is None else bias_abs[sl]))
    return {key: torch.cat([o[key] for o in outs]) for key in outs[0]}


def _attn_ref_chunk(q, k, v, do, scale, bias, bias_abs):
    N, d = q.shape[1:]
    tr = lambda t: t.transpose(-1, -2)
    s = scale * (q @ tr(k))
    a = scale * (q.abs() @ tr(k.abs()))
    if bias is not None:
        s = s + bias
        a = a + (bias.abs() if bias_abs is None else bias_abs)
    P = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    o = P @ v
    dP = do @ tr(v)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    r = dict(o=o, lse=lse, delta=delta.squeeze(-1), dS=dS, dq=scale * (dS @ k), dk=scale * (tr(dS) @ q), dv=tr(P) @ do)
    ds = c_f32(d) * U_F32 * (a + a.amax(-1, keepdim=True) + math.log(N))
    pds = (P * ds).sum(-1, keepdim=True)
    rel = ds + pds + c_f32(N) * U_F32
    av, ak, aq, ado = v.abs(), k.abs(), q.abs(), do.abs()
    om = P @ av
    dsm = P * (ado @ tr(av) + (ado * om).sum(-1, keepdim=True))
    dse = dsm * rel
    r.update(om=om, oext=(P * rel) @ av, lse_b=(pds.squeeze(-1) + c_f32(N) * U_F32) / math.log(2.0) + U_F32 * lse.abs(),
             deltam=(ado * om).sum(-1), deltaext=(ado * ((P * rel) @ av)).sum(-1),
             dsm=dsm, dsext=dse, dqm=scale * (dsm @ ak), dqext=scale * (dse @ ak), dkm=scale * (tr(dsm) @ aq), dkext=scale * (tr(dse) @ aq),
             dvm=tr(P) @ ado, dvext=tr(P * rel) @ ado)
    return r


def window_ref(qkv, dout, table, heads, ws, shift, keep):
    """The windowed attention of SwinTransformer.py (oracle/swin_oracle.py: roll, window_partition, relative_position_index,
    shift_mask) in fp64 through attn_ref.  qkv [B,H,W,3C], dout [B,H,W,C] fp64 on the device (processed an image at a time),
    table [(2ws-1)^2, heads].  Returns, for the images in `keep`, o / dqkv and their mags and ext terms as [len(keep),H,W,*] tensors,
    and dtable, its mag and ext summed over ALL images."""
    import swin_oracle as S
    B, H, W, C3 = qkv.shape
    C, N, dev = C3 // 3, ws * ws, qkv.device
    d, nW = C // heads, (H // ws) * (W // ws)
    rpi = S.relative_position_index(ws).reshape(-1).to(dev)
    bias = table[rpi].reshape(N, N, heads).permute(2, 0, 1)                           # [heads, N, N]
    mask = S.shift_mask(H, W, ws, shift).to(dev) if shift else torch.zeros(nW, N, N, dtype=torch.float64, device=dev)
    full = (bias[None] + mask[:, None]).reshape(nW * heads, N, N)
    fabs = (bias.abs()[None] + mask.abs()[:, None]).reshape(nW * heads, N, N)
    T2 = (2 * ws - 1) ** 2
    dtab = {k: torch.zeros(T2, heads, dtype=torch.float64, device=dev) for k in ("dS", "dsm", "dsext")}
    kept = {}

    def part(x):       # [1,H,W,c] -> [nW*heads, N, c/heads] for c = n*C: (n, heads) split
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        n = x.shape[-1] // C
        xw = S.window_partition(x, ws).reshape(nW, N, n, heads, d).permute(2, 0, 3, 1, 4)
        return xw.reshape(n, nW * heads, N, d)

    def unpart(t):     # [n][nW*heads, N, d] -> [1,H,W,n*C]
        n = len(t)
        x = torch.stack(t).reshape(n, nW, heads, N, d).permute(1, 3, 0, 2, 4).reshape(nW, ws, ws, n * C)
        x = S.window_reverse(x, ws, H, W)
        return torch.roll(x, shifts=(shift, shift), dims=(1, 2)) if shift else x

    for b in range(B):
        q, k, v = part(qkv[b:b + 1].double())
        (do,) = part(dout[b:b + 1].double())
        r = attn_ref(q, k, v, do, d ** -0.5, full, fabs)
        for key in dtab:
            dtab[key].index_add_(0, rpi, r[key].reshape(nW, heads, N * N).sum(0).T)
        if b in keep:
            kept[b] = dict(o=unpart([r["o"]]), om=unpart([r["om"]]), oext=unpart([r["oext"]]),
                           dqkv=unpart([r["dq"], r["dk"], r["dv"]]), dqkvm=unpart([r["dqm"], r["dkm"], r["dvm"]]),
                           dqkvext=unpart([r["dqext"], r["dkext"], r["dvext"]]))
    out = {key: torch.cat([kept[b][key] for b in keep]) for key in kept[keep[0]]}
    out.update(dtable=dtab["dS"], dtablem=dtab["dsm"], dtableext=dtab["dsext"])
    return out


def ln_wide_ref(x, dy, gamma, beta, eps=1e-5):
    """LayerNorm over the last axis (oracle/swin_oracle.py layer_norm, eps 1e-5) of x [M, C] fp64 on the device, its backward for dy,
    and the mags of test_gpu_norm_routes.py (no activation).  ext terms: the fp32 mean's rounding (2^-20*|mean|, amplified by rstd)
    enters xhat - it is what a row of zero variance shows."""
    import swin_oracle as S
    assert S.LN_EPS == eps
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = S.layer_norm(xr, gr, br)
    (y * dy).sum().backward()
    mu = x.mean(-1, keepdim=True)
    rstd = (((x - mu) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x - mu) * rstd
    xe = U_F32 * rstd * mu.abs()                              # error of the kernel's xhat from its fp32 mean
    gg = (gamma * dy).abs()
    mean = lambda t: t.mean(-1, keepdim=True)
    return dict(y=y.detach(), ymag=(gamma * xh).abs() + beta.abs(), yext=xe * gamma.abs(),
                dx=xr.grad, dxmag=rstd * (gg + mean(gg) + xh.abs() * mean(gg * xh.abs())),
                dgamma=gr.grad, dgmag=(dy * xh).abs().sum(0), dgext=(dy.abs() * xe).sum(0), dbeta=br.grad, dbmag=dy.abs().sum(0))
