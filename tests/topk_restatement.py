"""A float64 NumPy restatement of the top-k (hard-pixel) cross-entropy, written after the definition in include/usseg.h (``UssegTopkLoss``) -
not after the kernels.

On probabilities p[m][c] and labels y[m][c], m over the M pixels of the call:

    l(m)  = CategoricalCrossentropy(label_smoothing=0.1) of pixel m on probabilities (ys = y*0.9 + 0.1/C, q = p / sum_c p,
            -sum_c ys*log(clip(q, 1e-7, 1 - 1e-7)) with the fp32 values of the two clip constants)              [``pixel_loss``]
    key   = the uint32 bits of fp32 l with the sign bit cleared                                                 [``keys_of``]
    scope "batch": one segment of n = M pixels;  "image": M/HW segments of n = HW                              [``segments``]
    k     = max(1, min(n, floor(f * n))), f the fp32 fraction widened to double                                 [``k_of``]
    t = the k-th largest key, ngt = |{key > t}|, neq = |{key == t}|, r = k - ngt                                [``select``]
    a(m)  = 1 (key > t), r/neq (key == t), 0 (key < t)                                                          [``weights``]
    L_tk  = tk_weight * inv_global_batch * (n/k) * sum_m a(m)*l(m)                                              [``loss``]
    G_c(m) = tk_weight * inv_global_batch * (n/k) * a(m) * d l(m) / d p_c(m)                                    [``dlogits_terms``]

``loss`` and ``dlogits_terms`` take l as GIVEN (the fp64 values of ``pixel_loss``, or the fp32 values a kernel wrote): the selection is a
function of the fp32 bits, so a comparison that is to be free of near-threshold flips selects on the bits under test.
"""
import math

import numpy as np
import torch

import overlap_restatement as R

SCOPES = ("batch", "image")


def config(loss="topk", **kw):
    cfg = dict(fraction=0.1, scope="batch", tk_weight=1.0, dice=loss == "dice_topk")
    cfg.update(kw)
    return cfg


def k_of(f32, n):
    """k = max(1, min(n, floor((double)f * n))): the product of a 24-bit and a <= 30-bit number is exact in fp64."""
    f = float(np.float32(f32))
    v = math.floor(f * n) if math.isfinite(f) else 0
    return max(1, min(int(n), int(v)))


def pixel_loss(p, y):
    """l fp64 [M] from p, y [..., C] (any float type; evaluated in fp64)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, np.shape(p)[-1])
    y = np.asarray(y, dtype=np.float64).reshape(p.shape)
    C = p.shape[-1]
    ys = y * (1.0 - R.SMOOTH_LABEL) + R.SMOOTH_LABEL / C
    q = p / p.sum(-1, keepdims=True)
    return -(ys * np.log(np.clip(q, R.LO, R.HI))).sum(-1)


def keys_of(l32):
    return np.ascontiguousarray(l32, dtype=np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)


def select(keys_u32, k):
    """(t, ngt, neq) of ONE segment as exact integers."""
    keys = np.asarray(keys_u32, dtype=np.uint32).reshape(-1)
    n = keys.size
    assert 1 <= k <= n
    t = int(np.partition(keys, n - k)[n - k])
    return t, int((keys > t).sum()), int((keys == t).sum())


def weights(keys_u32, k):
    keys = np.asarray(keys_u32, dtype=np.uint32).reshape(-1)
    t, ngt, neq = select(keys, k)
    r = k - ngt
    assert 1 <= r <= neq
    return (keys > t).astype(np.float64) + (keys == t) * (r / neq)


def segments(M, HW, scope):
    """-> (S, n)."""
    assert scope in SCOPES and M % HW == 0
    return (M // HW, HW) if scope == "image" else (1, M)


def all_weights(l32, HW, cfg):
    """a [M] and the common k, n from the fp32 values of l."""
    keys = keys_of(l32)
    M = keys.size
    S, n = segments(M, HW, cfg["scope"])
    k = k_of(cfg["fraction"], n)
    a = np.concatenate([weights(keys[s * n:(s + 1) * n], k) for s in range(S)]) if M else np.zeros(0)
    return a, k, n


def loss(l, HW, cfg, inv_global_batch=1.0, l32=None):
    """L_tk from l (fp64 values summed; the selection on the bits of ``l32``, default l rounded to fp32)."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    if l.size == 0:
        return 0.0
    a, k, n = all_weights(l.astype(np.float32) if l32 is None else l32, HW, cfg)
    sel = a != 0.0                                      # (an unselected pixel contributes nothing, whatever its value)
    return cfg["tk_weight"] * inv_global_batch * (n / k) * float((a[sel] * l[sel]).sum())


def cce_grad(p, y):
    """d l(m) / d p_c(m), fp64 [M, C] (autograd of overlap_restatement.cce_per_pixel: zero where the quotient is clipped)."""
    pc = torch.as_tensor(np.asarray(p, dtype=np.float64)).reshape(-1, np.shape(p)[-1]).clone().requires_grad_(True)
    R.cce_per_pixel(pc, torch.as_tensor(np.asarray(y, dtype=np.float64)).reshape(pc.shape)).sum().backward()
    return pc.grad.numpy()


def dlogits_terms(p, y, a, k, n, cfg, inv_global_batch=1.0):
    """-> (G [M, C], dlogits [M, C], mag [M, C]): the top-k part of d loss / d p, what it gives through p_j*(G_j - sum_c p_c*G_c), and the
    magnitude of the terms for a per-element bound (tests/test_gpu_overlap_loss.py's construction)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, np.shape(p)[-1])
    G = cfg["tk_weight"] * inv_global_batch * (n / k) * np.asarray(a)[:, None] * cce_grad(p, y)
    dl = p * (G - (G * p).sum(-1, keepdims=True))
    S = np.abs(G)
    return G, dl, p * (S + (S * p).sum(-1, keepdims=True))
