"""A NumPy restatement of DataFilePlayGround.dataAug of the reference (:177-246) AS EXECUTED, and of the oversampling block it was written
for (:404-433), from the definitions in DESIGN.md section 4h - not from the kernels of csrc/prep_aug.hip.

A record is a float64 [H, W, Cc] array: channel 0 the label, 1..Cc-2 the displacement frames, Cc-1 the B-mode image.  The draws of one call
are a dict (the product's ``draw_aug`` makes the same one):
  flip, reduc, contrast, rotate, noise : bool      clip : (r, c, ra, ca) or None      shift : (r, c, direction) or None
  angle : degrees ((r % 11) / 5)                    seed : of the device's generated noise (unused here: the field is always given)

``rotate`` restates scipy.ndimage.rotate(img, angle, reshape=False) (order 3, mode='constant', cval=0, prefilter on): the cubic B-spline
prefilter with the mirror boundary along both axes, then per output pixel the 4x4 B-spline sum at R (i, j) + offset, 0 outside the image.
It takes a dtype so that the same steps can be evaluated in np.longdouble: the difference is the restatement's own rounding error.
"""
import math

import numpy as np
from scipy import special

F64 = np.float64
IPH = (8, 9, 10, 12, 22, 47, 53, 62, 66, 67, 69, 74, 75, 78, 85, 89, 93, 101, 105, 107, 110, 112, 113, 120, 121, 126, 129, 130, 133)
OFF = dict(flip=False, reduc=False, contrast=False, clip=None, rotate=False, angle=0.0, shift=None, noise=False, seed=0)


def params(**kw):
    """A forced parameter set: every step off except the ones given."""
    p = dict(OFF)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------------ percentile
def virtual_index(n, q):
    """numpy's position of the q-th percentile among n sorted values (method 'linear'): (n-1) * (q/100)."""
    pos = (n - 1) * (F64(q) / F64(100))
    k = int(math.floor(pos))
    return k, F64(pos - k)


def lerp(a, b, g):
    d = b - a
    return a + d * g if g < 0.5 else b - d * (1.0 - g)


def percentile(values, q):
    v = np.sort(np.asarray(values, F64).ravel())
    k, g = virtual_index(v.size, q)
    return lerp(v[k], v[min(k + 1, v.size - 1)], g)


# ------------------------------------------------------------------------------------------------ rotation
def prefilter(a, dtype=F64):
    """The cubic B-spline prefilter along axis 0 of ``a`` (mirror boundary); returns a new array of ``dtype``."""
    c = np.array(a, dtype=dtype)
    n = c.shape[0]
    z = np.sqrt(dtype(3)) - dtype(2)
    gain = (1 - z) * (1 - 1 / z)
    c *= gain
    zn1 = dtype(math.pow(float(z), n - 1)) if dtype is F64 else z ** (n - 1)
    zi = z
    c0 = c[0] + zn1 * c[n - 1]
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])        # = z^i c[i] + z^(2n-2-i') c[i'] with i' = n-1-i
        zi = zi * z
    c[0] = c0 / (1 - zn1 * zn1)
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def rotation(angle, H, W):
    """-> the six doubles (R00, R01, R10, R11, off0, off1) of scipy.ndimage.rotate(reshape=False) for an [H, W] plane."""
    c, s = F64(special.cosdg(angle)), F64(special.sindg(angle))
    R = np.array([[c, s], [-s, c]], F64)
    centre = (np.array([H, W], F64) - 1) / 2
    off = centre - R @ centre
    return (R[0, 0], R[0, 1], R[1, 0], R[1, 1], off[0], off[1])


def mirror(idx, n):
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx > n - 1, 2 * (n - 1) - idx, idx)


def rotate(img, angle, dtype=F64):
    """scipy.ndimage.rotate(img, angle, reshape=False) of an [H, W, C] array, evaluated in ``dtype``."""
    img = np.asarray(img, F64)
    H, W = img.shape[:2]
    coef = prefilter(img, dtype)
    coef = np.moveaxis(prefilter(np.moveaxis(coef, 1, 0), dtype), 0, 1)
    r00, r01, r10, r11, o0, o1 = (dtype(v) for v in rotation(angle, H, W))
    ii = np.arange(H).astype(dtype)[:, None]
    jj = np.arange(W).astype(dtype)[None, :]
    y = (ii * r00 + jj * r01) + o0
    x = (ii * r10 + jj * r11) + o1
    inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    y, x = np.where(inside, y, 0), np.where(inside, x, 0)
    fy, fx = np.floor(y), np.floor(x)

    def weights(t):
        u = 1 - t
        w1 = (t * t * (t - 2) * 3 + 4) / 6
        w2 = (u * u * (u - 2) * 3 + 4) / 6
        w0 = u * u * u / 6
        return [w0, w1, w2, 1 - w0 - w1 - w2]
    wy, wx = weights(y - fy), weights(x - fx)
    y0, x0 = fy.astype(np.int64) - 1, fx.astype(np.int64) - 1
    out = np.zeros(img.shape, dtype)
    for a in range(4):
        ya = mirror(y0 + a, H)
        for b in range(4):
            xb = mirror(x0 + b, W)
            out = out + (coef[ya, xb] * wy[a][..., None]) * wx[b][..., None]
    return np.where(inside[..., None], out, dtype(0))


# ------------------------------------------------------------------------------------------------ the other steps
def flip(img):
    return np.array(img[:, ::-1])


def reduc(img):
    """imageReduc on image[:, :, :-1] as executed: channels 1..Cc-2 are zeroed where the label is exactly 0."""
    out = np.array(img)
    out[:, :, 1:-1] = np.where(out[:, :, :1] == 0, 0.0, out[:, :, 1:-1])
    return out


def contrast(img):
    """The stretch, the percentile clip, the second stretch and the label gate; unchanged if hi == lo or maxval == minval."""
    out = np.array(img)
    S = out[:, :, 1:]
    lo, hi = S.min(), S.max()
    if hi == lo:
        return np.array(img)
    out[:, :, 1:] = (hi * (S - lo)) / (hi - lo)
    minval, maxval = percentile(out, 2), percentile(out, 98)
    if maxval == minval:
        return np.array(img)
    S = np.clip(out[:, :, 1:], minval, maxval)
    S = (maxval * (S - minval)) / (maxval - minval)
    out[:, :, 1:] = np.where(out[:, :, :1] < 0.1, 0.0, S)
    return out


def clip_box(img, box):
    r, c, ra, ca = box
    out = np.array(img)
    H, W = out.shape[:2]
    for i in range(H - 1):
        for j in range(W - 1):
            if r + ra > i > r - ra and c + ca > j > c - ca:
                out[i, j, :] = 0
    return out


def shift(img, sh):
    r, c, direction = sh
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    for i in range(H - 1):
        for j in range(W - 1):
            si, sj = (i + r, j + c) if direction else (i - r, j - c)
            if 0 <= si < H and 0 <= sj < W:
                out[i, j, :] = img[si, sj, :]
    return out


def add_noise(img, field):
    """field: the unit Gaussian [H, W, Cc-1]."""
    out = np.array(img)
    out[:, :, 1:] = out[:, :, 1:] + np.asarray(field, F64) / 5000.0
    return out


def dataAug(img, p, field=None, dtype=F64):
    """The whole chain on one record with the draws ``p``; ``field`` is needed iff p['noise'].  ``dtype``: of the rotation and what follows."""
    out = np.array(img, F64)
    if p["flip"]:
        out = flip(out)
    if p["reduc"]:
        out = reduc(out)
    if p["contrast"]:
        out = contrast(out)
    if p["clip"] is not None:
        out = clip_box(out, p["clip"])
    if p["rotate"]:
        out = rotate(out, p["angle"], dtype)
    if p["shift"] is not None:
        out = shift(out, p["shift"])
    if p["noise"]:
        out = add_noise(out, field)
    return out


# ------------------------------------------------------------------------------------------------ the oversampling plan
def bleed_fraction(img):
    return np.count_nonzero(img[:, :, 0] >= 1.05) / (img.shape[0] * img.shape[1])


def plan(name, patient, f, mode):
    """-> [(row name, 'reduc' | 'aug')] appended after a TRAINING record ``name`` of bleed fraction f; mode None | 'bleed' | 'all'."""
    rows = []
    if mode is None:
        return rows
    if patient in IPH:
        rows += [(name + "iph_%d" % x, "reduc") for x in range(2)]
    if f > 0.05:
        rows += [(name + "_%d" % y, "aug") for y in range(math.floor(f / 0.03))]
    if mode == "all":
        rows += [(name + "aug_%d" % z, "aug") for z in range(2)]
    return rows


def record(rng, H=24, W=20, Cc=12, bleed=True):
    """A synthetic record: an elliptic brain (label 1, outside 0), a blurred-looking bleed blob (label up to 2), frames zero outside the
    brain, a B-mode channel that is never zero."""
    yy, xx = np.mgrid[0:H, 0:W]
    inside = ((yy - H / 2) / (0.42 * H)) ** 2 + ((xx - W / 2) / (0.45 * W)) ** 2 < 1
    img = rng.standard_normal((H, W, Cc)) * 0.3
    label = np.where(inside, 1.0, 0.0)
    if bleed:
        d = ((yy - H * 0.4) / (0.15 * H)) ** 2 + ((xx - W * 0.55) / (0.2 * W)) ** 2
        label = np.where(inside, np.maximum(label, np.clip(2.2 - d, 1.0, 2.0)), 0.0)
    img[:, :, 0] = label.astype(np.float32)
    img[:, :, 1:-1] *= inside[..., None]
    img[:, :, -1] = rng.uniform(-2.0, -0.1, (H, W))
    return img
