"""A float64 restatement of the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018; batch-level, ``per_image=False``), written after the
definition in include/usseg.h (``UssegLovaszLoss``) - not after the kernels.

Per class c, on probabilities p[m][c] (fp32 values) and labels y[m][c], m over the M pixels of the call:

    fg(m) = y_c(m) > threshold                       (a NaN is not foreground)
    e(m)  = fg ? 1 - p_c(m) : p_c(m)                 (ONE fp32 operation: numpy float32 gives the kernel's bits)
    key   = the uint32 bits of |e|, clamped to 0x3F800000
    order = key descending, ties by ascending pixel index
    r = 0-based rank, F = foreground pixels of rank <= r, Y = sum fg, I = Y - F, U = Y + r + 1 - F
    g = 1/U (foreground), I/(U*(U-1)) (background);  Y = 0: g = 1 at rank 0, else 0          [``grad_closed``]
    L_c = sum_m e(m)*g(m)

``grad_paper`` is the listing of the paper (Alg. 1: the differences of the Jaccard losses of the sorted prefix sets), kept beside the closed form.

    L_lv = (1/|S|) * sum_{c in S} w[c]*L_c,  S = the classes with Y_c > 0 ("present") or all classes ("all"); an empty S gives 0
    loss = ce_weight * CCE + lv_weight * ov_scale * L_lv          (CCE: overlap_restatement.cce_per_pixel, times inv_global_batch)
    d loss / d p_c(m) = k_c * (fg ? -1 : +1) * g_c(m) (+ the CCE term),  k_c = lv_weight*ov_scale*w[c]/|S| in S, 0 outside
"""
import numpy as np
import torch

import overlap_restatement as R

ONE_BITS = 0x3F800000
KEY_BITS = 30


def config(loss="lovasz", C=3, **kw):
    """loss name -> settings as the model's constructor resolves them."""
    cfg = dict(w=[1.0] * C, lv_weight=1.0, ce_weight=1.0 if loss == "lovasz_ce" else 0.0, threshold=0.5, classes="present")
    cfg.update(kw)
    return cfg


def foreground(y, threshold=0.5):
    return np.asarray(y, dtype=np.float64) > threshold               # (a comparison with NaN is False)


def errors32(p32, fg):
    """e as the kernel forms it: float32 in, one float32 subtraction."""
    p32 = np.asarray(p32, dtype=np.float32)
    return np.where(fg, np.float32(1.0) - p32, p32).astype(np.float32)


def keys(e32):
    b = np.ascontiguousarray(e32, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.minimum(b, np.uint32(ONE_BITS))


def order(key):
    """The permutation 'key descending, ties by ascending index' of ONE class: perm[r] = the pixel of rank r."""
    return np.argsort((ONE_BITS - key.astype(np.int64)), kind="stable")


def grad_closed(fg_sorted):
    """g along the sorted order from the exact integers (fp64 only in the final division)."""
    fg_sorted = np.asarray(fg_sorted, dtype=bool)
    n = fg_sorted.size
    Y = int(fg_sorted.sum())
    if Y == 0:
        g = np.zeros(n)
        g[:1] = 1.0
        return g
    r = np.arange(n, dtype=np.int64)
    F = np.cumsum(fg_sorted.astype(np.int64))
    I, U = Y - F, Y + r + 1 - F
    return np.where(fg_sorted, 1.0 / U, I / np.maximum(U * (U - 1), 1).astype(np.float64))


def grad_paper(fg_sorted):
    """Alg. 1 of the paper: jaccard = 1 - intersection/union of the sorted prefixes, then its first differences."""
    gt = np.asarray(fg_sorted, dtype=np.float64)
    gts = gt.sum()
    inter = gts - np.cumsum(gt)
    union = gts + np.cumsum(1.0 - gt)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return jac


def coeffs(p32, y, threshold=0.5):
    """-> (g fp64 [M, C] in PIXEL order, counts int64 [C], rank int64 [M, C]) at fp32 probabilities [..., C]."""
    C = p32.shape[-1]
    p = np.asarray(p32, dtype=np.float32).reshape(-1, C)
    fg = foreground(np.asarray(y).reshape(-1, C), threshold)
    g = np.zeros(p.shape)
    rank = np.zeros(p.shape, dtype=np.int64)
    for c in range(C):
        perm = order(keys(errors32(p[:, c], fg[:, c])))
        g[perm, c] = grad_closed(fg[perm, c])
        rank[perm, c] = np.arange(perm.size)
    return g, fg.sum(0).astype(np.int64), rank


def class_set(counts, cfg):
    """S: every class, or the classes with a foreground pixel."""
    return [c for c in range(len(counts)) if cfg["classes"] == "all" or counts[c] > 0]


def per_class(p, y, cfg):
    """L_c (fp64 tensor [C], differentiable in the fp64 tensor ``p`` whose values are fp32 numbers), g, counts.  The order is taken at p's
    values and held constant: L_c is linear in p on the piece the order defines."""
    C = p.shape[-1]
    g, counts, _ = coeffs(p.detach().numpy().astype(np.float32), y.numpy(), cfg["threshold"])
    fg = torch.from_numpy(foreground(y.numpy().reshape(-1, C), cfg["threshold"]))
    p2 = p.reshape(-1, C)
    e = torch.where(fg, 1.0 - p2, p2)
    return (e * torch.from_numpy(g)).sum(0), g, counts


def k_coefficients(counts, cfg, ov_scale=1.0):
    S = class_set(counts, cfg)
    k = np.zeros(len(counts))
    for c in S:
        k[c] = cfg["lv_weight"] * ov_scale * cfg["w"][c] / len(S)
    return k


def loss(p, y, cfg, inv_global_batch=1.0, ov_scale=1.0):
    """The scalar loss (fp64 tensor, differentiable in p)."""
    Lc, _, counts = per_class(p, y, cfg)
    if p.numel() == 0:
        return torch.zeros((), dtype=torch.float64)
    k = torch.from_numpy(k_coefficients(counts, cfg, ov_scale))
    out = (k * Lc).sum()
    if cfg["ce_weight"] != 0.0:
        out = out + cfg["ce_weight"] * inv_global_batch * R.cce_per_pixel(p, y).sum()
    return out


def restate_at(p32, y, cfg, inv_global_batch=1.0, ov_scale=1.0):
    """Everything the GPU tests compare against, at GIVEN fp32 probabilities (torch [..., C]): loss, L_c, g, counts, k, G = d loss / d p and S, the
    sizes of G's terms |k_c|*g (+ |CCE term|)."""
    p = p32.double().cpu().clone().requires_grad_(True)
    y = y.double().cpu()
    l = loss(p, y, cfg, inv_global_batch, ov_scale)
    l.backward()
    Lc, g, counts = per_class(p.detach(), y, cfg)
    k = k_coefficients(counts, cfg, ov_scale)
    S = torch.from_numpy(np.abs(k) * g).reshape(p.shape)
    if cfg["ce_weight"] != 0.0:
        pc = p.detach().clone().requires_grad_(True)
        (cfg["ce_weight"] * inv_global_batch * R.cce_per_pixel(pc, y).sum()).backward()
        S = S + pc.grad.abs()
    return dict(loss=l.item(), L=Lc.detach(), g=g.reshape(p.shape), counts=counts, k=k, G=p.grad, S=S)


KINDS = ("gauss", "quantised", "saturated", "absent", "full")


def inputs(kind="gauss", C=3, B=2, H=9, W=7, seed=77):
    """(logits, y) fp64 tensors with fp32-representable values.  gauss: overlap_restatement.inputs (logits from N(0, 2^2); image 0 one-hot, the others
    soft labels) - a few dozen tied keys per class at 2x256x80; quantised: the logits rounded to multiples of 2, a handful of distinct
    probabilities and so ties everywhere; saturated: logits from N(0, 30^2), most probabilities exactly 0 or 1; absent: the last class is nowhere
    foreground; full: class 0 is foreground at every pixel (and so no other class anywhere)."""
    logits, y = R.inputs(C, B, H, W, seed)
    if kind == "quantised":
        logits = 2.0 * torch.round(logits / 2.0)
    elif kind == "saturated":
        logits = (15.0 * logits).float().double()
    elif kind == "absent":
        y = y.clone()
        y[..., C - 1] = torch.minimum(y[..., C - 1], torch.tensor(0.25, dtype=torch.float64))
    elif kind == "full":
        y = torch.zeros_like(y)
        y[..., 0] = 1.0
    elif kind != "gauss":
        raise ValueError(kind)
    return logits, y


def ties(p32, y, threshold=0.5):
    """Per class, the number of pixels whose key some other pixel shares."""
    C = p32.shape[-1]
    p = np.asarray(p32, dtype=np.float32).reshape(-1, C)
    fg = foreground(np.asarray(y).reshape(-1, C), threshold)
    out = []
    for c in range(C):
        _, cnt = np.unique(keys(errors32(p[:, c], fg[:, c])), return_counts=True)
        out.append(int(cnt[cnt > 1].sum()))
    return out
