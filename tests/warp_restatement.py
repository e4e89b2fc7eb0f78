"""NumPy fp64 restatement of ``usseg_elastic_warp`` (include/usseg.h; csrc/warp.hip), in the stated order of every operation, for bit-for-bit
comparisons: the hash in wrapping ``uint64``, the separable zero-padded blur, the source coordinates, the bilinear image and nearest label
sampling, and the copy of inactive samples.  NumPy evaluates ``a + w * u`` as a rounded product followed by a rounded sum (no fused
multiply-add), which is what the kernels are compiled to."""
import numpy as np

M1, M2, GOLDEN = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53), np.uint64(0x9e3779b97f4a7c15)
S33 = np.uint64(33)


def aug_hash(v):
    """The low 32 bits of the 64-bit finaliser of csrc/common.h (``aug_hash``); ``v``: a uint64 ARRAY (array arithmetic wraps silently)."""
    v = np.asarray(v, dtype=np.uint64).copy()
    v ^= v >> S33
    v *= M1
    v ^= v >> S33
    v *= M2
    v ^= v >> S33
    return (v & np.uint64(0xffffffff)).astype(np.uint32)


def field(seed, H, W):
    """u [2,H,W] fp64 = h * 2^-31 - 1, h = aug_hash(seed * GOLDEN + ((k*H + i)*W + j)): uniform on [-1, 1), exact."""
    ctr = np.arange(2 * H * W, dtype=np.uint64) + np.array([int(seed) & ((1 << 64) - 1)], dtype=np.uint64) * GOLDEN
    return (aug_hash(ctr).astype(np.float64) * 2.0 ** -31 - 1.0).reshape(2, H, W)


def blur_axis(u, w, axis):
    """s[p] = sum over k = -radius..radius ASCENDING of w[|k|] * u[p + k] along ``axis``, from +0.0, taps outside skipped; radius 0: u itself."""
    r = len(w) - 1
    if r == 0:
        return u.copy()
    u = np.moveaxis(u, axis, -1)
    n = u.shape[-1]
    acc = np.zeros_like(u)
    for k in range(-r, r + 1):
        lo, hi = max(0, -k), min(n, n - k)            # p in [lo, hi): 0 <= p + k < n
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + w[abs(k)] * u[..., lo + k:hi + k]
    return np.moveaxis(acc, -1, axis)


def smooth(u, w):
    """[..., H, W]: along H, then along W."""
    return blur_axis(blur_axis(u, w, -2), w, -1)


def coordinates(disp, aff, H, W):
    """src [2,H,W]: ((A00*i + A01*j) + o0) + disp0 and ((A10*i + A11*j) + o1) + disp1, each operation rounded."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a = [np.float64(v) for v in aff]
    return np.stack([((a[0] * i + a[1] * j) + a[4]) + disp[0], ((a[2] * i + a[3] * j) + a[5]) + disp[1]])


def bilinear(x, src):
    """x [H,W,C] -> fp64 [H,W,C]: ((w00*v00 + w01*v01) + w10*v10) + w11*v11, a tap outside the image 0, a coordinate that is not finite or not
    inside (-1, H) x (-1, W) gives 0."""
    H, W, _ = x.shape
    with np.errstate(invalid="ignore"):
        inside = (src[0] > -1.0) & (src[0] < H) & (src[1] > -1.0) & (src[1] < W)
    s0, s1 = np.where(inside, src[0], 0.0), np.where(inside, src[1], 0.0)
    fi, fj = np.floor(s0), np.floor(s1)
    f0, f1 = s0 - fi, s1 - fj
    g0, g1 = 1.0 - f0, 1.0 - f1
    ti, tj = fi.astype(np.int64), fj.astype(np.int64)
    xd = x.astype(np.float64)

    def tap(a, b):
        ok = (a >= 0) & (a < H) & (b >= 0) & (b < W)
        return np.where(ok[..., None], xd[np.clip(a, 0, H - 1), np.clip(b, 0, W - 1)], 0.0)
    e = lambda t: t[..., None]
    out = ((e(g0 * g1) * tap(ti, tj) + e(g0 * f1) * tap(ti, tj + 1)) + e(f0 * g1) * tap(ti + 1, tj)) + e(f0 * f1) * tap(ti + 1, tj + 1)
    return np.where(inside[..., None], out, 0.0)


def nearest(y, src):
    """y [H,W] -> y[floor(src0 + 0.5)][floor(src1 + 0.5)], 0 outside (and for a coordinate that is not finite)."""
    H, W = y.shape
    n0, n1 = np.floor(src[0] + 0.5), np.floor(src[1] + 0.5)
    with np.errstate(invalid="ignore"):
        ok = (n0 >= 0) & (n0 < H) & (n1 >= 0) & (n1 < W)
    a, b = np.where(ok, n0, 0).astype(np.int64), np.where(ok, n1, 0).astype(np.int64)
    return np.where(ok, y[a, b], np.float32(0)).astype(y.dtype)


def warp(x, y, params, w, fld=None):
    """x [B,H,W,C] fp32 / fp64, y [B,H,W] fp32, ``params`` the ``draw_warp`` dicts, ``w`` the weight table, ``fld`` an injected field [B,2,H,W] or
    None -> (x_out, y_out, disp [B,2,H,W], field_used [B,2,H,W]); an inactive sample is copied bit for bit and its disp and field are 0."""
    B, H, W, _ = x.shape
    xo, yo = x.copy(), y.copy()
    disp, used = np.zeros((B, 2, H, W)), np.zeros((B, 2, H, W))
    for b, p in enumerate(params):
        if not p["active"]:
            continue
        used[b] = field(p["seed"], H, W) if fld is None else fld[b]
        s = smooth(used[b], w)
        disp[b] = np.stack([np.float64(p["alpha"][0]) * s[0], np.float64(p["alpha"][1]) * s[1]])
        src = coordinates(disp[b], p["aff"], H, W)
        xo[b] = bilinear(x[b], src).astype(x.dtype)               # rounded once
        yo[b] = nearest(y[b], src)
    return xo, yo, disp, used
