"""NumPy restatement of csrc/ensemble.hip (include/usseg.h, "ensemble prediction, uncertainty maps and calibration counters").

fp64 versions of the three kernels, each with the magnitude its error bound is stated against (the sum of the absolute terms), and fp32
versions of the two results that must match bit for bit: the sequential mean of the members and the calibration quantisation
(``np.rint`` in fp32: half to even, as ``rintf``).  The comparison rules are the kernels': a first maximum never moves to a NaN, a term
with p <= 0 contributes 0, a NaN propagates, and a negative difference is clamped to 0 while a NaN stays.
"""
import numpy as np

Q = np.float32(2.0 ** 24)


def unflip(members, flip_w):
    """The members as the merge reads them: member k mirrored along W when bit k of flip_w is set."""
    return [np.ascontiguousarray(m[:, :, ::-1]) if (flip_w >> k) & 1 else m for k, m in enumerate(members)]


def mean_f32(members, flip_w=0):
    """(((p_0 + p_1) + ...) + p_(K-1)) / (float)K in fp32, members in ascending k."""
    ms = [np.asarray(m, np.float32) for m in unflip(members, flip_w)]
    acc = ms[0].copy()
    for m in ms[1:]:
        acc = (acc + m).astype(np.float32)
    return (acc / np.float32(len(ms))).astype(np.float32)


def plogp(p):
    """t(p) = p*log(p) for p > 0, 0 for p <= 0, NaN for a NaN (fp64)."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = p * np.log(np.where(p > 0, p, 1.0))
    return np.where(p > 0, t, np.where(p <= 0, 0.0, np.nan))


def clamp0(d):
    return np.where(d < 0, 0.0, d)


def merge(members, flip_w=0):
    """-> dict of fp64 arrays: mean [B,H,W,C], entropy, mutual_info [B,H,W], variance [B,H,W,C], and ``mag_*``: the sum of the absolute
    terms of entropy (|t(mean_c)|), mutual_info (those plus |t(p_kc)|/K) and variance (sum p^2/K + mean^2)."""
    ms = np.stack([np.asarray(m, np.float64) for m in unflip(members, flip_w)])     # [K,B,H,W,C]
    K = ms.shape[0]
    mean = ms.sum(0) / K
    tm = plogp(mean)
    tk = plogp(ms)
    H = -tm.sum(-1)
    EH = -tk.sum((0, -1)) / K
    sq = (ms * ms).sum(0) / K
    return dict(mean=mean, entropy=H, mutual_info=clamp0(H - EH), variance=clamp0(sq - mean * mean),
                mag_entropy=np.abs(tm).sum(-1), mag_mutual_info=np.abs(tm).sum(-1) + np.abs(tk).sum((0, -1)) / K,
                mag_variance=sq + mean * mean)


def first_max(a):
    """Index of the first maximum along the last axis; a NaN is never larger (and an all-NaN row gives 0)."""
    a = np.asarray(a)
    arg = np.zeros(a.shape[:-1], np.int64)
    best = a[..., 0].copy()
    for c in range(1, a.shape[-1]):
        with np.errstate(invalid="ignore"):
            take = a[..., c] > best
        best = np.where(take, a[..., c], best)
        arg = np.where(take, c, arg)
    return arg, best


def image_scores(mean_probs, entropy, mutual_info):
    """-> (scores fp64 [B,4], counts int64 [B], mag fp64 [B,4]) from the maps as given (pass the device's maps to bound the sums alone)."""
    mean_probs, e, m = np.asarray(mean_probs), np.asarray(entropy, np.float64), np.asarray(mutual_info, np.float64)
    B = e.shape[0]
    arg, _ = first_max(mean_probs)
    last = (arg == mean_probs.shape[-1] - 1).reshape(B, -1)
    e, m = e.reshape(B, -1), m.reshape(B, -1)
    n = last.sum(1)
    scores = np.zeros((B, 4))
    mag = np.zeros((B, 4))
    scores[:, 0], mag[:, 0] = e.mean(1), np.abs(e).mean(1)
    scores[:, 1], mag[:, 1] = m.mean(1), np.abs(m).mean(1)
    scores[:, 2] = m.max(1)                                   # np.max keeps a NaN, as the kernel does
    mag[:, 2] = np.abs(scores[:, 2])
    sel, sel_abs = (e * last).sum(1), (np.abs(e) * last).sum(1)
    scores[:, 3] = np.where(n > 0, sel / np.maximum(n, 1), 0.0)
    mag[:, 3] = np.where(n > 0, sel_abs / np.maximum(n, 1), 0.0)
    return scores, n.astype(np.int64), mag


def calibration(probs, y_true, bins, cls=-1):
    """-> (counts int64 [bins*3 + 2] with the per-bin counters and the invalid count exact and the Brier slot the fp32-quantised sum of this
    restatement's fp64 v, brier_f64: sum v * 2^24 in fp64, n_valid).  conf, the bin index and rint(conf * 2^24) are fp32, as in the kernel."""
    p = np.asarray(probs, np.float32).reshape(-1, np.shape(probs)[-1])
    t = np.asarray(y_true, np.float32).reshape(p.shape)
    C = p.shape[1]
    ap, pbest = first_max(p)
    at, _ = first_max(t)
    if cls < 0:
        conf, hit = pbest.astype(np.float32), ap == at
    else:
        conf, hit = p[:, cls], at == cls
    with np.errstate(invalid="ignore"):
        valid = (conf >= 0) & (conf <= 1)
    cv = np.where(valid, conf, np.float32(0)).astype(np.float32)
    b = np.minimum(bins - 1, (cv * np.float32(bins)).astype(np.float32).astype(np.int64))
    q = np.rint((cv * Q).astype(np.float32)).astype(np.int64)
    counts = np.zeros(bins * 3 + 2, np.int64)
    np.add.at(counts, b[valid] * 3, 1)
    np.add.at(counts, b[valid & hit] * 3 + 1, 1)
    np.add.at(counts, b[valid] * 3 + 2, q[valid])
    onehot = np.eye(C)[at]
    v = ((p.astype(np.float64) - onehot) ** 2).sum(1)
    with np.errstate(invalid="ignore"):
        v = np.where(v <= C, v, float(C))
    brier = float((v[valid] * 2.0 ** 24).sum())
    counts[bins * 3] = int(np.rint(v[valid] * 2.0 ** 24).sum())
    counts[bins * 3 + 1] = int((~valid).sum())
    return counts, brier, int(valid.sum())


def scores_from_counts(counts):
    """ECE, MCE, Brier and the reliability table from a counter block, in fp64 (metrics.calibration_from_counts restated)."""
    counts = np.asarray(counts, np.int64)
    bins = (counts.size - 2) // 3
    t = counts[:bins * 3].reshape(bins, 3).astype(np.float64)
    n = t[:, 0]
    N = n.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(n > 0, t[:, 1] / n, 0.0)
        conf = np.where(n > 0, t[:, 2] / 2.0 ** 24 / n, 0.0)
    gap = np.abs(acc - conf)
    ece = float((n / N * gap).sum()) if N > 0 else float("nan")
    mce = float(gap[n > 0].max()) if N > 0 else float("nan")
    brier = float(counts[bins * 3] / 2.0 ** 24 / N) if N > 0 else float("nan")
    return dict(n=n.astype(np.int64), accuracy=acc, confidence=conf, ece=ece, mce=mce, brier=brier, n_invalid=int(counts[bins * 3 + 1]))
