"""A float64 torch restatement of the region-overlap losses (soft Dice / Tversky, optionally plus CategoricalCrossentropy), written after
the definition in include/usseg.h (``UssegOverlapLoss``) - not after the kernels.

On probabilities p[m][c] and labels y[m][c] as passed (no label smoothing in the overlap term), m over the M pixels of the call:

    I_c = sum_m p*y      P_c = sum_m p      Y_c = sum_m y
    N_c = I_c + s        D_c = (1-a-b)*I_c + a*P_c + b*Y_c + s        T_c = N_c / D_c
    L_ov = sum_c w_c * (1 - T_c)^g
    loss = ce_weight * CCE + ov_weight * ov_scale * L_ov

CCE is Keras' CategoricalCrossentropy(label_smoothing=0.1) on probabilities, summed over the pixels and times ``inv_global_batch``:
ys = y*0.9 + 0.1/C, q = p / sum_c p, -sum_c ys*log(clip(q, 1e-7, 1 - 1e-7)) with the fp32 values of the two clip constants.
"""
import numpy as np
import torch

LO = float(np.float32(1e-7))
HI = float(np.float32(1.0 - 1e-7))
SMOOTH_LABEL = 0.1

# loss name -> settings as the model's constructor resolves them (class weights uniform)
def config(loss, C=3, **kw):
    a, b = (0.3, 0.7) if loss == "tversky" else (0.5, 0.5)
    cfg = dict(w=[1.0 / C] * C, alpha=a, beta=b, smooth=1.0, power=1.0, ov_weight=1.0, ce_weight=1.0 if loss == "dice_ce" else 0.0)
    cfg.update(kw)
    return cfg


def sums(p, y):
    """I, P, Y per class (fp64) over every leading axis."""
    C = p.shape[-1]
    p, y = p.double().reshape(-1, C), y.double().reshape(-1, C)
    return (p * y).sum(0), p.sum(0), y.sum(0)


def tversky(I, P, Y, alpha, beta, smooth):
    N = I + smooth
    D = (1.0 - alpha - beta) * I + alpha * P + beta * Y + smooth
    return N, D, N / D


def coefficients(I, P, Y, cfg, ov_scale=1.0):
    """A_c, B_c of d loss / d p_c(m) = A_c*y_c(m) + B_c, by the stated formulas."""
    a, b, g = cfg["alpha"], cfg["beta"], cfg["power"]
    N, D, T = tversky(I, P, Y, a, b, cfg["smooth"])
    w = torch.as_tensor(cfg["w"], dtype=torch.float64)
    k = cfg["ov_weight"] * ov_scale * w * g * (1.0 - T) ** (g - 1.0)
    return -k * (D - (1.0 - a - b) * N) / D ** 2, k * a * N / D ** 2


def cce_per_pixel(p, y):
    """Keras CategoricalCrossentropy(label_smoothing=0.1, reduction NONE) on probabilities -> [...]."""
    C = p.shape[-1]
    ys = y.double() * (1.0 - SMOOTH_LABEL) + SMOOTH_LABEL / C
    q = p.double() / p.double().sum(-1, keepdim=True)
    return -(ys * torch.log(torch.clamp(q, LO, HI))).sum(-1)


def overlap_term(p, y, cfg):
    """L_ov (fp64 scalar tensor, differentiable in p)."""
    I, P, Y = sums(p, y)
    _, _, T = tversky(I, P, Y, cfg["alpha"], cfg["beta"], cfg["smooth"])
    w = torch.as_tensor(cfg["w"], dtype=torch.float64)
    return (w * (1.0 - T) ** cfg["power"]).sum()


def loss(p, y, cfg, inv_global_batch=1.0, ov_scale=1.0):
    out = cfg["ov_weight"] * ov_scale * overlap_term(p, y, cfg)
    if cfg["ce_weight"] != 0.0:
        out = out + cfg["ce_weight"] * inv_global_batch * cce_per_pixel(p, y).sum()
    return out


def inputs(C=3, B=2, H=9, W=7, seed=77):
    """The inputs of the kernel tests: fp32-representable logits from N(0, 2^2) and labels - image 0 one-hot, the others soft."""
    gen = torch.Generator().manual_seed(seed + 31 * C + H * W)
    logits = (2.0 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)).float().double()
    y = torch.softmax(2.0 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float64), -1).float().double()
    y[0] = torch.nn.functional.one_hot(y[0].argmax(-1), C).double()
    return logits, y


def from_logits(logits, y, cfg, inv_global_batch=1.0, ov_scale=1.0):
    """softmax -> loss, as the launches run it.  -> dict: probs, loss, dlogits (autograd), G (autograd at the probabilities), I / P / Y / T /
    A / B, mag (the magnitude of the per-element dlogits bound) and edge (pixels with a normalised probability within 2^-20 relative of a CCE
    clip constant, where fp32 may clip and fp64 not; all False without a CCE term).

    mag[k] = p[k]*(S[k] + sum_c S[c]*p[c]) with S[c] = |A_c|*|y_c| + |B_c| + |d CCE term / d p_c|: the sizes of the TERMS that make up
    G_c = A_c*y_c + B_c (+ CCE) and then p[k]*(G[k] - sum_c G[c]*p[c]).  A_c <= 0 <= B_c, so G_c itself may cancel; an error in a coefficient is
    relative to the terms, not to their difference."""
    z = logits.double().clone().requires_grad_(True)
    p = torch.softmax(z, -1)
    p.retain_grad()
    l = loss(p, y, cfg, inv_global_batch, ov_scale)
    l.backward()
    pd = p.detach()
    I, P, Y = sums(pd, y)
    _, D, T = tversky(I, P, Y, cfg["alpha"], cfg["beta"], cfg["smooth"])
    A, B = coefficients(I, P, Y, cfg, ov_scale)
    S = A.abs() * y.double().abs() + B.abs()
    edge = torch.zeros(pd.shape[:-1], dtype=torch.bool)
    if cfg["ce_weight"] != 0.0:
        pc = pd.clone().requires_grad_(True)
        (cfg["ce_weight"] * inv_global_batch * cce_per_pixel(pc, y).sum()).backward()
        S = S + pc.grad.abs()
        rel = 2.0 ** -20
        q = pd / pd.sum(-1, keepdim=True)
        edge = (((q - LO).abs() <= rel * LO) | ((q - HI).abs() <= rel * HI)).any(-1)
    mag = pd * (S + (S * pd).sum(-1, keepdim=True))
    return dict(probs=pd, loss=l.detach(), dlogits=z.grad, G=p.grad, I=I, P=P, Y=Y, T=T, D=D, A=A, B=B, mag=mag, edge=edge)


def sum_depth(M):
    """The longest chain of fp32 additions behind one of the kernel's totals, from the grid rule usseg.h states: grid = clamp(ceil(ceil(M/4)/256),
    1, 512) workgroups of 256 threads; a thread adds its groups of four pixels in order (4 additions per group), a wave its 64 lanes by a
    butterfly (6), a workgroup its four waves as a tree (2); the last workgroup adds every sixteenth workgroup in order (ceil(grid/16)) and the
    sixteen strands as a tree (4).  Plus one for the rounding of the product p*y."""
    groups = (M + 3) // 4
    grid = min(max((groups + 255) // 256, 1), 512)
    iters = (groups + grid * 256 - 1) // (grid * 256)
    return 4 * iters + 6 + 2 + (grid + 15) // 16 + 4 + 1, grid


def sum_bound(M):
    """Relative error bound of a total of NON-NEGATIVE terms summed in fp32 along chains of at most d roundings: gamma_d = d*u / (1 - d*u), u = 2^-24."""
    d, _ = sum_depth(M)
    u = 2.0 ** -24
    return d * u / (1.0 - d * u)
