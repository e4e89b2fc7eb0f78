"""A restatement of the surface order statistics and the surface Dice, written after the definitions in include/usseg.h
(``usseg_surface_stats``) - not after the kernels - on top of tests/boundary_restatement.py's brute-force squared distance transform.

Per image: the SORTED integer squared distances of the three sets D_ab, D_ba and D_pool (empty when either surface is empty), and

    pos = q / 100 * (n - 1)     k = floor(pos)     k1 = min(k + 1, n - 1)     g = pos - k
    value = sqrt(d2[k]) + (sqrt(d2[k1]) - sqrt(d2[k])) * g

in plain Python floats: the same IEEE operations, in the same order, as the host code (``metrics.surface_scores_from_stats``), so the tests
compare bits.  pooled = the value of D_pool; directed = the larger of the values of D_ab and D_ba; NaN where either surface is empty.
Surface Dice at tau: (|{D_ab <= t2}| + |{D_ba <= t2}|) / (|S(a)| + |S(b)|), t2 the largest integer with sqrt(t2) <= tau; NaN where both surfaces are
empty, 0.0 where exactly one is.
"""
import math
from fractions import Fraction

import numpy as np

from boundary_restatement import surface_counters


def sets(a, b):
    """One image -> (counters [|S(a)|, |S(b)|, max_ab, max_ba], [sorted D_ab, sorted D_ba, sorted D_pool]) as int64 arrays."""
    c, dab, dba = surface_counters(a, b)
    d_ab = np.sort(np.rint(dab * dab).astype(np.int64))        # boundary_restatement returns the roots of exact integers
    d_ba = np.sort(np.rint(dba * dba).astype(np.int64))
    return c, [d_ab, d_ba, np.sort(np.concatenate([d_ab, d_ba]))]


def ranks(q, n):
    """-> (pos, k, k1) for a set of n >= 1."""
    pos = q / 100 * (n - 1)
    k = math.floor(pos)
    return pos, k, min(k + 1, n - 1)


def pair(q, d2):
    """The two squared distances the device returns for one sorted set: (-1, -1) when it is empty."""
    if len(d2) == 0:
        return (-1, -1)
    _, k, k1 = ranks(q, len(d2))
    return (int(d2[k]), int(d2[k1]))


def percentile(q, d2):
    """The order statistic of one sorted set of squared distances, in pixels; NaN for an empty set."""
    if len(d2) == 0:
        return float("nan")
    pos, k, k1 = ranks(q, len(d2))
    g = pos - k
    lo, hi = math.sqrt(int(d2[k])), math.sqrt(int(d2[k1]))
    return lo + (hi - lo) * g


def tol2(tau):
    """The largest integer m whose fp64 square root, ``math.sqrt(m)`` - the distance as it is reported - is <= tau: a search upwards from below
    floor(tau^2) (exact rational arithmetic) with the comparison itself."""
    m = max(math.floor(Fraction(tau) ** 2) - 2, 0)
    assert math.sqrt(m) <= tau
    while math.sqrt(m + 1) <= tau:
        m += 1
    return m


def scores(a, b, percentiles=(), tolerances=()):
    """One image -> dict(counters, sel [3][P] pairs, within [T] pairs, pooled [P], directed [P], nsd [T])."""
    c, d = sets(a, b)
    sel = [[pair(q, s) for q in percentiles] for s in d]
    within = [(int((d[0] <= tol2(t)).sum()), int((d[1] <= tol2(t)).sum())) for t in tolerances]
    pooled = [percentile(q, d[2]) for q in percentiles]
    directed = [max(percentile(q, d[0]), percentile(q, d[1])) if len(d[2]) else float("nan") for q in percentiles]
    den = c[0] + c[1]
    nsd = [(w[0] + w[1]) / den if den else float("nan") for w in within]
    return dict(counters=c, sets=d, sel=sel, within=within, pooled=pooled, directed=directed, nsd=nsd)
