"""A float64 / float32 NumPy restatement of the offline preprocessing (DataFilePlayGround.output2DImages of the reference, mode 1), written
from the cv2 rules the product restates - not from its kernels - plus a writer of small synthetic raw trees.

cv2 rules (a restatement; cv2 is not installed, so they were not checked against it):
  resize INTER_LINEAR, per axis: scale = 1/(dsize/ssize); f = float32((d+0.5)*scale - 0.5); s = floor(f); f -= s (float32);
    s < 0 -> (0, 0); s >= ssize-1 -> (ssize-1, 0) and one horizontal tap.  Weights float32 (1-f, f).  Horizontal pass, then vertical
    b0*row(s) + b1*row(min(s+1, ssize-1)).  float64 data: weights applied in double; float32 data: all float32.
  GaussianBlur(k, sigma), float32: t = float32(exp(-x^2/(2 sigma^2))), w = float32(t * (1/sum t)); rows then columns, ordered sums,
    BORDER_REFLECT_101.
  INTER_AREA: box averages when no axis grows, else linear with the area coefficients (restated in test_cpu_prep.py's known answers).
"""
import math
import os

import numpy as np

F32, F64 = np.float32, np.float64
H_OUT, W_OUT = 256, 80
BAD = (1, 14, 22, 23, 27, 28, 32, 34, 35, 36, 37, 38, 39, 44, 49, 69, 71, 78, 82, 90, 98, 101, 121, 124, 128, 133, 136, 928)


def lin_axis(dsize, ssize):
    """-> (s0, s1, w0, w1, two) arrays over the dsize output coordinates."""
    inv = dsize / ssize
    scale = 1.0 / inv
    d = np.arange(dsize, dtype=F64)
    f = ((d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    neg = s < 0
    s[neg], f[neg] = 0, F32(0)
    hi = s >= ssize - 1
    s[hi], f[hi] = ssize - 1, F32(0)
    s1 = np.minimum(s + 1, ssize - 1)
    return s, s1, (F32(1) - f).astype(F32), f, ~hi


def resize_linear(src, dsize=(H_OUT, W_OUT)):
    """cv2.resize(src, (W, H)) INTER_LINEAR of [H,W] or [H,W,C] float64 / float32 data."""
    src = np.asarray(src)
    dt = src.dtype
    assert dt in (F32, F64)
    ex = (lambda a: a[:, None]) if src.ndim == 3 else (lambda a: a)
    ys0, ys1, b0, b1, _ = lin_axis(dsize[0], src.shape[0])
    xs0, xs1, a0, a1, two = lin_axis(dsize[1], src.shape[1])
    a0, a1, b0, b1 = (w.astype(dt) for w in (a0, a1, b0, b1))
    with np.errstate(invalid="ignore"):
        both = src[:, xs0] * ex(a0) + src[:, xs1] * ex(a1)
        hor = np.where(ex(two)[None], both, src[:, xs0])
        out = hor[ys0] * ex(b0[:, None]) + hor[ys1] * ex(b1[:, None])
    return out.astype(dt)


def gauss_kernel(k, sigma):
    scale2 = -0.5 / (sigma * sigma)
    t = [F32(math.exp(scale2 * x * x)) for x in (i - (k - 1) * 0.5 for i in range(k))]
    s = 0.0
    for v in t:
        s += float(v)
    s = 1.0 / s
    return np.array([F32(float(v) * s) for v in t], F32)


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.array(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
    return p


def gaussian_blur(img, k, sigma):
    img = np.asarray(img, F32)
    w = gauss_kernel(k, sigma)
    H, W = img.shape
    r = k // 2
    rows = np.zeros_like(img)
    for i in range(k):
        rows = (rows + w[i] * img[:, reflect101(np.arange(W) + i - r, W)]).astype(F32)
    out = np.zeros_like(img)
    for i in range(k):
        out = (out + w[i] * rows[reflect101(np.arange(H) + i - r, H)]).astype(F32)
    return out


def label_and_gate(brain, blood, normal, objective):
    """-> (label float32 [256,80], gate bool [256,80]) as :330-343."""
    brain_r = resize_linear(np.asarray(brain, F64))
    gate = brain_r == 0
    if objective == 0:
        return np.where(gate, 0, 1).astype(F32), gate
    blood, normal = np.asarray(blood, F64), np.asarray(normal, F64)
    with np.errstate(invalid="ignore"):
        b = blood > normal
    lab = np.where(b, 2, 1).astype(F32)
    lab = gaussian_blur(lab, 9, 4)
    lab = np.where(b, F32(2), lab).astype(F32)
    lab = gaussian_blur(lab, 3, 2)
    lab = np.where(b, F32(2), lab).astype(F32)
    lab = resize_linear(lab)
    return np.where(gate, F32(0), lab).astype(F32), gate


def normalise(x):
    x = x - x.mean(axis=0).mean(axis=0)
    safe = np.abs(x).max(axis=0).max(axis=0)
    safe[safe == 0] = 1
    return x / safe


def process_file(mat, objective):
    """One loaded file (dict of arrays) -> float64 [C,1,256,80,12] as :286-393 (mode 1)."""
    disp = np.asarray(mat["displacement"], F64)
    hr = np.asarray(mat["hrTimes"], F64)
    label, gate = label_and_gate(mat["brainMask"], mat["bloodMask"], mat["normalMask"], objective)
    with np.errstate(divide="ignore"):
        bmode = np.log10(np.asarray(mat["bModeNorm"], F64)).mean(axis=2)
    out = []
    for h in range(hr.shape[1] - 1):
        start = int(math.ceil(30 * hr[0, h]))
        real = resize_linear(normalise(disp[:, :, start:start + 5]))
        imag = resize_linear(normalise(disp[:, :, start + 5:start + 10]))
        if objective == 1:
            real[gate], imag[gate] = 0.0, 0.0
        with np.errstate(invalid="ignore"):
            b = resize_linear(np.ascontiguousarray(bmode[:, :, h]))
        out.append([np.concatenate([label[..., None].astype(F64), real, imag, b[..., None]], axis=2)])
    return np.array(out).reshape(-1, 1, H_OUT, W_OUT, 12)


def driver(iteration, objective, raw, seed):
    """The whole of output2DImages in one process (sorted files within a patient) -> (train, test, train_paths, test_paths)."""
    from scipy.io import loadmat
    names = np.sort(os.listdir(raw))
    names = names[np.random.RandomState(20).permutation(len(names))]
    tr, te, trp, tep = [], [], [], []
    for count, name in enumerate(names):
        if int(name[-3:]) in BAD:
            continue
        for f in sorted(os.listdir(os.path.join(raw, name))):
            if ".mat" not in f:
                continue
            imgs = process_file(loadmat(os.path.join(raw, name, f)), objective)
            for img in imgs:
                if count % 10 == iteration % 10:
                    te.append(img), tep.append([f[0:17]])
                else:
                    tr.append(img), trp.append([f[0:17]])

    def shuf(rows, paths, s):
        p = np.random.RandomState(s).permutation(len(rows))
        data = np.array(rows).reshape(-1, 1, H_OUT, W_OUT, 12)[p]
        return data, np.array(paths, dtype=str).reshape(-1, 1)[p]
    train, train_paths = shuf(tr, trp, seed)
    test, test_paths = shuf(te, tep, seed // 17)
    return train, test, train_paths, test_paths


# ------------------------------------------------------------------------------------------------ synthetic raw data
def make_mat(rng, H0=37, W0=23, C=3, T=None, Hq=None, Wq=None, F=3, Hm=None, Wm=None, Hb=None, Wb=None, nan_blood=True, zero_channel=False,
             log_zero=False, axis=False):
    """One synthetic file: a dict ready for scipy.io.savemat."""
    Hm, Wm = Hm or H0, Wm or W0
    Hb, Wb = Hb or Hm, Wb or Wm
    Hq, Wq = Hq or H0, Wq or W0
    starts = [3 + 11 * h for h in range(C)]
    T = T or starts[-1] + 10 + 2
    hr = np.array([[(s - 0.5) / 30 for s in starts] + [(starts[-1] + 20) / 30]])      # ceil(30 * t) == s
    disp = rng.standard_normal((H0, W0, T)) * 1e-3 + rng.standard_normal(T) * 1e-4
    if zero_channel:
        disp[:, :, starts[0] + 2] = 0.0                      # an all-zero plane: safe_max = 1
    bmode = rng.uniform(0.01, 1.0, (Hq, Wq, F, C + 1))
    if log_zero:
        bmode[Hq // 2, Wq // 3, 0, 0] = 0.0                   # log10(0) = -inf
    yy, xx = np.mgrid[0:Hb, 0:Wb]
    brain = (((yy - Hb / 2) / (0.4 * Hb)) ** 2 + ((xx - Wb / 2) / (0.45 * Wb)) ** 2 < 1).astype(F64)
    normal = rng.uniform(0, 1, (Hm, Wm))
    blood = rng.uniform(0, 1, (Hm, Wm)) * 0.8
    blood[Hm // 3:Hm // 2, Wm // 4:Wm // 2] += 0.6
    if nan_blood:
        blood[rng.uniform(size=(Hm, Wm)) < 0.1] = np.nan
        normal[0, 0] = np.nan
    m = {"displacement": disp, "hrTimes": hr, "bModeNorm": bmode, "brainMask": brain, "bloodMask": blood, "normalMask": normal}
    if axis:
        m["xAxis"] = np.linspace(-40, 40, H0 * W0).reshape(H0, W0)
        m["zAxis"] = np.linspace(0, 120, H0 * W0).reshape(W0, H0).T.copy()
    return m


def write_tree(root, seed=0, patients=12, files=(1, 2), cycles=(2, 4), size=(37, 23)):
    """DoD001 .. DoD0NN (DoD001 is a bad patient) with 1-2 .mat files each and 2-4 cycles per file; returns the root."""
    from scipy.io import savemat
    rng = np.random.default_rng(seed)
    for p in range(1, patients + 1):
        d = os.path.join(root, "DoD%03d" % p)
        os.makedirs(d)
        for f in range(int(rng.integers(files[0], files[1] + 1))):
            m = make_mat(rng, H0=size[0], W0=size[1], C=int(rng.integers(cycles[0], cycles[1] + 1)), axis=True)
            savemat(os.path.join(d, "DoD%03d_Ter%03d_RC%d_Displacement_Polar.mat" % (p, f + 1, p % 3)), m)
    return root
