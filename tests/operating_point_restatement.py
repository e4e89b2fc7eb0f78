"""NumPy restatement of csrc/operating_point.hip (include/usseg.h, "threshold sweeps and temperature scaling") and of the host arithmetic on
its counters (metrics.sweep_from_counts, metrics.temperature_search).  Integers and fp64; the fp32 steps whose rounding decides an integer
(the bin of a score, the quantised NLL) are taken in fp32.  Nothing here imports the package."""
import math

import numpy as np

EPS = np.float32(1e-7)            # the CCE's epsilon
UNIT = 2.0 ** 20                  # counts per unit of NLL
CAP = 1024.0


def first_max(y):
    """The first-maximum class along the last axis; a NaN is never larger (so an all-NaN pixel is class 0)."""
    y = np.asarray(y)
    at = np.zeros(y.shape[:-1], np.int64)
    best = y[..., 0].copy()
    for c in range(1, y.shape[-1]):
        with np.errstate(invalid="ignore"):
            more = y[..., c] > best
        at[more] = c
        best = np.where(more, y[..., c], best)
    return at


# ------------------------------------------------------------------------------------------------ the sweep
def sweep_bins(s, bins):
    """fp32 scores -> (bin int64, valid bool): bin = min(bins-1, (int)(s*(float)bins)) in fp32, clamped at 0; invalid = NaN or outside [0, 1]."""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        valid = (s >= 0) & (s <= 1)
    prod = np.where(valid, s, np.float32(0)) * np.float32(bins)          # an fp32 product
    b = np.clip(prod.astype(np.int64), 0, bins - 1)                      # astype truncates towards zero, as (int) does
    return b, valid


def sweep_counts(probs, y, bins, cls):
    """-> int64 [2*bins + 1]: per bin (negatives, positives) of class ``cls`` (0..C-1), then the invalid pixels."""
    probs, y = np.asarray(probs, np.float32), np.asarray(y, np.float32)
    C = probs.shape[-1]
    s = probs.reshape(-1, C)[:, cls]
    pos = first_max(y.reshape(-1, C)) == cls
    b, valid = sweep_bins(s, bins)
    out = np.zeros(2 * bins + 1, np.int64)
    np.add.at(out, (2 * b + pos)[valid], 1)
    out[2 * bins] = int((~valid).sum())
    return out


def thresholds(bins):
    """threshold[k], k = 0..bins: -inf, the largest fp32 below k/bins, and 1.0 at k = bins (s = 1 lies in the last bin: nothing is >= bin `bins`)."""
    t = [-math.inf]
    for k in range(1, bins):
        t.append(float(np.nextafter(np.float32(k / bins), np.float32(0))))
    t.append(1.0)
    return np.array(t, np.float32)


def sweep_from_counts(counts):
    """Pure-Python restatement of metrics.sweep_from_counts: lists and Python numbers."""
    c = [int(v) for v in counts]
    bins = (len(c) - 1) // 2
    neg, pos = c[0:2 * bins:2], c[1:2 * bins:2]
    P, N = sum(pos), sum(neg)
    nan = float("nan")
    out = dict(tp=[], fp=[], fn=[], tn=[], tpr=[], fpr=[], precision=[], dice=[])
    for k in range(bins + 1):
        tp, fp = sum(pos[k:]), sum(neg[k:])
        fn, tn = P - tp, N - fp
        out["tp"].append(tp); out["fp"].append(fp); out["fn"].append(fn); out["tn"].append(tn)
        out["tpr"].append(tp / P if P else nan)
        out["fpr"].append(fp / N if N else nan)
        out["precision"].append(tp / (tp + fp) if tp + fp else 1.0)
        out["dice"].append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    num = sum(pos[b] * (2 * sum(neg[:b]) + neg[b]) for b in range(bins))
    out["auc"] = num / (2 * P * N) if P and N else nan
    out["average_precision"] = sum((out["tp"][k] - out["tp"][k + 1]) * out["precision"][k] for k in range(bins)) / P if P else nan
    thr = thresholds(bins)
    out["threshold"] = thr

    def best(v):
        if any(math.isnan(x) for x in v):
            return 0, float(thr[0]), float(v[0])
        top = max(v)
        k = v.index(top)                  # the smallest k
        return k, float(thr[k]), float(top)
    out["best_dice"] = best(out["dice"])
    out["best_youden"] = best([a - b for a, b in zip(out["tpr"], out["fpr"])])
    out["n_invalid"] = c[2 * bins]
    return out


# ------------------------------------------------------------------------------------------------ the temperature
def _valid_pixels(flat):
    with np.errstate(invalid="ignore"):
        return ((flat >= 0) & (flat <= 1)).all(-1)


def nll(probs, y, betas):
    """-> (nll fp64 [M_valid, n]: the exact per-pixel NLL of each fp32 beta, T fp64 [M_valid, n]: max_c |beta*z_c| (the bound's magnitude),
    n_valid, n_invalid).  z_c = log(p_c + float32(1e-7)) in fp64."""
    probs, y = np.asarray(probs, np.float32), np.asarray(y, np.float32)
    C = probs.shape[-1]
    flat = probs.reshape(-1, C)
    valid = _valid_pixels(flat)
    z = np.log(flat[valid].astype(np.float64) + float(EPS))
    lab = first_max(y.reshape(-1, C))[valid]
    b = np.array([float(np.float32(v)) for v in betas])
    t = z[:, None, :] * b[None, :, None]                                   # [M, n, C]
    m = t.max(-1)
    lse = m + np.log(np.exp(t - m[..., None]).sum(-1))
    ty = np.take_along_axis(t, lab[:, None, None].repeat(len(b), 1), 2)[..., 0]
    return lse - ty, np.abs(t).max(-1), int(valid.sum()), int((~valid).sum())


def nll_counts_f32(probs, y, betas):
    """The integer counters as an fp32 evaluation with NumPy's own logf / expf gives them (NOT bit-equal to the device's: its logf and expf
    differ in the last place): int64 [n + 2].  Used by the pure-Python search on the host."""
    probs, y = np.asarray(probs, np.float32), np.asarray(y, np.float32)
    C = probs.shape[-1]
    flat = probs.reshape(-1, C)
    valid = _valid_pixels(flat)
    z = np.log(flat[valid] + EPS).astype(np.float32)
    lab = first_max(y.reshape(-1, C))[valid]
    out = []
    for beta in betas:
        beta = np.float32(beta)
        t = (beta * z).astype(np.float32)
        m = t.max(-1)
        s = np.zeros(len(t), np.float32)
        for c in range(C):
            e = np.exp((t[:, c] - m).astype(np.float32)).astype(np.float32)
            s = e if c == 0 else (s + e).astype(np.float32)
        v = ((m + np.log(s).astype(np.float32)).astype(np.float32) - t[np.arange(len(t)), lab]).astype(np.float32)
        v = np.minimum(np.maximum(v, np.float32(0)), np.float32(CAP))
        out.append(int(np.rint(v.astype(np.float32) * np.float32(UNIT)).astype(np.int64).sum()))
    return out + [int(valid.sum()), int((~valid).sum())]


def nll_pixel_bound(T, beta, C, L, X):
    """The bound on |device nll_j - exact nll_j| of one pixel in COUNTS (units of 2^-20), to first order in u = 2^-24, with T = max_c |beta*z_c|,
    L / X the ulp errors of the device's logf / expf (|error| <= L * 2u * |value|):
        z_c:      the rounding of p_c + eps moves log by u, logf adds 2Lu|z_c|            -> |dz| <= u(1 + 2L|z_c|)
        t_c:      beta*z_c rounds once                                                     -> |dt| <= u(beta + (2L + 1)T) =: Dt, and |dm| <= Dt
        d_c:      t_c - m rounds once, |d_c| <= 2T                                          -> |dd| <= 2Dt + 2uT
        e_c:      expf adds 2Xu e_c to e_c*|dd|;  S: C-1 roundings of at most uS            -> |dS|/S <= 2Dt + 2uT + 2Xu + (C-1)u
        log S:    logf adds 2Lu log C                                                       -> |dls| <= |dS|/S + 2Lu log C
        a = m+ls: one rounding, |a| <= T + log C;  nll = a - t_y: one rounding, |nll| <= 2T + log C
        total:    u[4 beta + (8L + 9)T + 2X + C - 1 + (2L + 2) log C]
    and half a count for the quantisation.  The clamp at 0 only moves a value towards the exact one (which is >= 0)."""
    u = 2.0 ** -24
    first = u * (4 * beta + (8 * L + 9) * T + 2 * X + C - 1 + (2 * L + 2) * math.log(C if C > 1 else 2))
    return first * (1 + 2.0 ** -10) * UNIT + 0.5                 # (1 + 2^-10): the second-order terms


def apply_temperature(probs, beta):
    """fp64 softmax(beta * log(p + float32(1e-7))) per pixel; a pixel with a NaN z is NaN in every class."""
    probs = np.asarray(probs, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = float(np.float32(beta)) * np.log(probs.astype(np.float64) + float(EPS))
    bad = np.isnan(t).any(-1)
    t = np.where(bad[..., None], 0.0, t)
    e = np.exp(t - t.max(-1, keepdims=True))
    out = e / e.sum(-1, keepdims=True)
    out[bad] = np.nan
    return out


def f32(v):
    return float(np.float32(v))


def candidates(lo, hi, n, geometric):
    if geometric:
        return [f32(lo * (hi / lo) ** (i / (n - 1))) for i in range(n)]
    return [f32(lo + (hi - lo) * (i / (n - 1))) for i in range(n)]


def search(evaluate, lo=1 / 8, hi=8.0, n=16, rounds=4):
    """The bracket search over ``evaluate(betas) -> [sums..., n_valid, n_invalid]``: -> (beta, sum, sum at 1, final-round spacing)."""
    a, b = float(lo), float(hi)
    spacing = None
    for r in range(rounds):
        betas = candidates(a, b, n, r == 0)
        sums = [int(v) for v in evaluate(betas)][:n]
        i = 0
        for j in range(1, n):
            if sums[j] < sums[i] or (sums[j] == sums[i] and betas[j] < betas[i]):
                i = j
        if r == 0 and i in (0, n - 1):
            raise ValueError("edge")
        spacing = max(betas[j + 1] - betas[j] for j in range(n - 1))
        beta, best = betas[i], sums[i]
        a, b = betas[max(i - 1, 0)], betas[min(i + 1, n - 1)]
        if not a < b:
            break
    at1 = int(evaluate([1.0])[0])
    if at1 < best:
        beta, best = 1.0, at1
    return beta, best, at1, spacing


def dense_search(probs, y, lo=1 / 8, hi=8.0, points=20001):
    """The fp64 minimiser of the mean NLL on a dense geometric grid (the grid's ratio is 1 + 2e-4: far below a final-round spacing)."""
    probs, y = np.asarray(probs, np.float32), np.asarray(y, np.float32)
    C = probs.shape[-1]
    flat = probs.reshape(-1, C)
    valid = _valid_pixels(flat)
    z = np.log(flat[valid].astype(np.float64) + float(EPS))
    lab = first_max(y.reshape(-1, C))[valid]
    zy = z[np.arange(len(z)), lab]
    grid = lo * (hi / lo) ** (np.arange(points) / (points - 1))
    best, arg = None, None
    for chunk in np.array_split(grid, 50):
        t = z[None] * chunk[:, None, None]
        m = t.max(-1)
        v = (m + np.log(np.exp(t - m[..., None]).sum(-1)) - chunk[:, None] * zy[None]).sum(-1)
        k = int(v.argmin())
        if best is None or v[k] < best:
            best, arg = float(v[k]), float(chunk[k])
    return arg
