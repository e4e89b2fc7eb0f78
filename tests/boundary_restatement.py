"""A float64 NumPy restatement of the distance maps and the boundary term, written after the definitions in include/usseg.h
(``usseg_sdf_labels``, ``usseg_surface_dist``, ``UssegBoundaryLoss``) - not after the kernels.

Squared distance transform: for every pixel the minimum over ALL target pixels of dy^2 + dx^2, by brute force, in int64 (the loop takes the
target pixels a row at a time so that a 256 x 80 plane needs megabytes, not gigabytes; nothing is pruned).

    mask = y_c > thr (NaN compares false: outside)          d(A) = sqrt of the squared transform towards A
    phi  = d(mask) outside the mask,  1 - d(not mask) inside,  0 everywhere for a class that is absent from or fills the plane

Surfaces: S(m) = mask pixels with a 4-neighbour outside the mask, out-of-image counting as outside.  Counters per image: |S(a)|, |S(b)|, max over
S(a) of the squared distance to S(b), the same from b to a (-1 each when either surface is empty), and the lists of (unsquared) distances.

Boundary term, on top of tests/overlap_restatement.py:  L_B = wb * ov_scale / M * sum_m sum_c u_c * p_c(m) * phi_c(m).
"""
import math

import numpy as np
import torch

import overlap_restatement as R


def sq_transform(target):
    """target bool [H,W] -> int64 [H,W]: min over the target pixels (r, q) of (y-r)^2 + (x-q)^2; -1 everywhere if there is none."""
    target = np.asarray(target, dtype=bool)
    H, W = target.shape
    big = np.iinfo(np.int64).max
    best = np.full((H, W), big, dtype=np.int64)
    ys = np.arange(H, dtype=np.int64)[:, None]
    xs = np.arange(W, dtype=np.int64)
    for r in range(H):
        q = np.flatnonzero(target[r]).astype(np.int64)
        if q.size == 0:
            continue
        dx2 = ((xs[:, None] - q[None, :]) ** 2).min(axis=1)            # [W]: every target pixel of row r
        np.minimum(best, (ys - r) ** 2 + dx2[None, :], out=best)
    if not target.any():
        return np.full((H, W), -1, dtype=np.int64)
    return best


def mask_of(y, thr=0.5):
    with np.errstate(invalid="ignore"):
        return np.asarray(y) > thr                                      # NaN > thr is False


def phi_plane(mask):
    """One plane's signed distance map in fp64."""
    mask = np.asarray(mask, dtype=bool)
    if not mask.any() or mask.all():
        return np.zeros(mask.shape, dtype=np.float64)
    out = np.sqrt(sq_transform(mask).astype(np.float64))
    inside = 1.0 - np.sqrt(sq_transform(~mask).astype(np.float64))
    return np.where(mask, inside, out)


def phi(y, thr=0.5):
    """y [B,H,W,C] -> phi fp64 [B,H,W,C]."""
    y = np.asarray(y)
    out = np.zeros(y.shape, dtype=np.float64)
    for b in range(y.shape[0]):
        for c in range(y.shape[-1]):
            out[b, :, :, c] = phi_plane(mask_of(y[b, :, :, c], thr))
    return out


def surface(m):
    """bool [H,W] -> the mask pixels with at least one 4-neighbour outside the mask (or outside the image)."""
    m = np.asarray(m) != 0
    p = np.pad(m, 1, constant_values=False)
    core = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~core


def surface_counters(a, b):
    """One image -> (counters [|S(a)|, |S(b)|, max_ab, max_ba], distances a -> b, distances b -> a) with the distances fp64 arrays (empty when
    either surface is empty, the maxima then -1)."""
    sa, sb = surface(a), surface(b)
    na, nb = int(sa.sum()), int(sb.sum())
    if na == 0 or nb == 0:
        return [na, nb, -1, -1], np.zeros(0), np.zeros(0)
    d_ab = sq_transform(sb)[sa]
    d_ba = sq_transform(sa)[sb]
    return [na, nb, int(d_ab.max()), int(d_ba.max())], np.sqrt(d_ab.astype(np.float64)), np.sqrt(d_ba.astype(np.float64))


def surface_scores(a, b):
    """One image -> (hd, assd) as defined in usseg.h; NaN where a surface is empty."""
    c, dab, dba = surface_counters(a, b)
    if c[0] == 0 or c[1] == 0:
        return float("nan"), float("nan")
    return math.sqrt(max(c[2], c[3])), 0.5 * (math.fsum(dab) / c[0] + math.fsum(dba) / c[1])


# ------------------------------------------------------------------------------------------------ the boundary term
def default_u(C):
    return [0.0] + [1.0] * (C - 1)


def boundary_term(p, phi_, u, wb, ov_scale=1.0):
    """L_B (fp64 scalar tensor, differentiable in p); p, phi_ [..., C]."""
    C = p.shape[-1]
    M = p.numel() // C
    uu = torch.as_tensor(u, dtype=torch.float64)
    return wb * ov_scale / M * (uu * p.double() * torch.as_tensor(phi_, dtype=torch.float64)).sum()


def loss(p, y, phi_, cfg, u, wb, inv_global_batch=1.0, ov_scale=1.0):
    return R.loss(p, y, cfg, inv_global_batch, ov_scale) + boundary_term(p, phi_, u, wb, ov_scale)


def restate_at(p32, y, phi_, cfg, u, wb, inv, ov_scale):
    """Loss, L_B, G = d loss / d p (autograd) and dlogits = p*(G - sum_c p_c*G_c) at GIVEN fp32 probabilities, in fp64; ``mag``: the sizes of the
    terms of G carried through that formula (tests/overlap_restatement.py's rule, plus |kb*u_c*phi_c| for the boundary summand); ``edge`` as there."""
    p = p32.double().cpu().clone().requires_grad_(True)
    phi_ = torch.as_tensor(phi_, dtype=torch.float64)
    l = loss(p, y, phi_, cfg, u, wb, inv, ov_scale)
    l.backward()
    pd = p.detach()
    G = p.grad
    I, P, Y = R.sums(pd, y)
    _, D, _ = R.tversky(I, P, Y, cfg["alpha"], cfg["beta"], cfg["smooth"])
    A, B = R.coefficients(I, P, Y, cfg, ov_scale)
    C = pd.shape[-1]
    M = pd.numel() // C
    kb = wb * ov_scale / M
    S = A.abs() * y.double().abs() + B.abs() + kb * torch.as_tensor(u, dtype=torch.float64) * phi_.abs()
    edge = torch.zeros(pd.shape[:-1], dtype=torch.bool)
    if cfg["ce_weight"] != 0.0:
        pc = pd.clone().requires_grad_(True)
        (cfg["ce_weight"] * inv * R.cce_per_pixel(pc, y).sum()).backward()
        S = S + pc.grad.abs()
        q = pd / pd.sum(-1, keepdim=True)
        rel = 2.0 ** -20
        edge = (((q - R.LO).abs() <= rel * R.LO) | ((q - R.HI).abs() <= rel * R.HI)).any(-1)
    mag = pd * (S + (S * pd).sum(-1, keepdim=True))
    ref = pd * (G - (G * pd).sum(-1, keepdim=True))
    lb = boundary_term(pd, phi_, u, wb, ov_scale).item()
    abs_terms = (kb * (torch.as_tensor(u, dtype=torch.float64) * pd * phi_.abs()).sum()).item()      # sum of |terms| of L_B
    return dict(loss=l.item(), lb=lb, lb_abs=abs_terms, kb=kb, G=G, dlogits=ref, mag=mag, edge=edge, D=D)


def labels(C, B, H, W, seed=5):
    """Labels for the loss tests: image 0 one-hot blobs (class c a disc), the others soft (a softmax of smooth fields), fp32-representable."""
    g = torch.Generator().manual_seed(seed + 17 * C + H * W)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    z = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    for c in range(1, C):
        cy, cx, r = H * (0.25 + 0.2 * c), W * (0.3 + 0.15 * c), 0.12 * min(H, W) * (1 + c)
        z[..., c] += 4.0 * ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).double()
    y = torch.softmax(2.0 * z, -1).float().double()
    y[0] = torch.nn.functional.one_hot(y[0].argmax(-1), C).double()
    return y
