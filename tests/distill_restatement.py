"""A float64 torch restatement of the knowledge-distillation loss, written line by line after the definition in include/usseg_distill.h -
not after the kernel.

    soften(r)_c = softmax_c( log(r_c + 1e-7) / T )                         pT = soften(p), qT = soften(q)
    soft(pixel) = T^2 * sum_c qT_c * (log qT_c - log pT_c)                 the logs as s_c - logsumexp(s)
    hard(pixel) = CategoricalCrossentropy(label_smoothing = 0.1, clip 1e-7)     (overlap_restatement.cce_per_pixel)
    loss        = scale * ( hard_weight * sum_pixels hard + soft_weight * sum_pixels soft )

Gradient with respect to the logits of p = softmax(z), soft term:   r_c = T*(pT_c - qT_c)*p_c/(p_c + 1e-7),   dz_j = r_j - p_j * sum_c r_c.
"""
import torch

import overlap_restatement as R

EPS = 1e-7
DEFAULTS = dict(temperature=2.0, soft_weight=0.5, hard_weight=0.5)


def soften(r, T):
    """-> (r_T, log r_T), fp64."""
    s = torch.log(r.double() + EPS) / T
    lg = s - torch.logsumexp(s, -1, keepdim=True)
    return torch.exp(lg), lg


def soft_per_pixel(p, q, T):
    pT, lp = soften(p, T)
    qT, lq = soften(q, T)
    return T * T * (qT * (lq - lp)).sum(-1)


def hard_per_pixel(p, y):
    return R.cce_per_pixel(p, y)


def loss(p, y, q, T, soft_weight, hard_weight, scale):
    """-> (loss, sum_pixels hard, sum_pixels soft), differentiable in p."""
    hard, soft = hard_per_pixel(p, y).sum(), soft_per_pixel(p, q, T).sum()
    return scale * (hard_weight * hard + soft_weight * soft), hard, soft


def soft_dlogits(p, q, T):
    """The closed form of d (sum_pixels soft) / d logits at probabilities p (unweighted, unscaled)."""
    p = p.double()
    pT, _ = soften(p, T)
    qT, _ = soften(q, T)
    r = T * (pT - qT) * p / (p + EPS)
    return r - p * r.sum(-1, keepdim=True)


def hard_G(p, y):
    """d (sum_pixels hard) / d p by autograd."""
    pc = p.double().clone().requires_grad_(True)
    hard_per_pixel(pc, y).sum().backward()
    return pc.grad


def at_probs(p, y, q, T, soft_weight, hard_weight, scale):
    """Everything the kernel tests compare with, at GIVEN probabilities p (fp64 arithmetic): loss, hard and soft sums, dlogits (closed form:
    the hard term's G through p_j*(G_j - sum_c p_c*G_c), plus the soft term's), mag and edge.

    mag = p * (S + sum_c S_c p_c),  S_c = hard_weight*scale*|dCCE/dp_c| + soft_weight*scale*T*(pT_c + qT_c)/(p_c + 1e-7): the sizes of the
    TERMS behind G_c (pT_c - qT_c may cancel: an error in either is relative to the term, not to the difference).
    edge: pixels with a normalised probability within 2^-20 relative of a CCE clip constant, where fp32 may clip and fp64 not."""
    p, y, q = p.double(), y.double(), q.double()
    l, hard, soft = loss(p, y, q, T, soft_weight, hard_weight, scale)
    Gh = hard_G(p, y)
    dl = hard_weight * scale * p * (Gh - (Gh * p).sum(-1, keepdim=True)) + soft_weight * scale * soft_dlogits(p, q, T)
    pT, _ = soften(p, T)
    qT, _ = soften(q, T)
    S = hard_weight * scale * Gh.abs() + soft_weight * scale * T * (pT + qT) / (p + EPS)
    mag = p * (S + (S * p).sum(-1, keepdim=True))
    n = p / p.sum(-1, keepdim=True)
    rel = 2.0 ** -20
    edge = (((n - R.LO).abs() <= rel * R.LO) | ((n - R.HI).abs() <= rel * R.HI)).any(-1)
    return dict(loss=l.item(), hard=hard.item(), soft=soft.item(), dlogits=dl, mag=mag, edge=edge)


def inputs(C=3, B=2, H=9, W=7):
    """Student logits and labels: ``overlap_restatement.inputs``.  The teacher's probabilities: a second draw (another seed, logits times 1.5),
    rounded to fp32.  -> (logits fp64, y fp64, q fp32)."""
    logits, y = R.inputs(C, B, H, W)
    tl, _ = R.inputs(C, B, H, W, seed=1077)
    q = torch.softmax(1.5 * tl, -1).float()
    return logits, y, q


def probs32(logits):
    """fp32 probabilities as the head leaves them (the restatement is then taken at THESE probabilities)."""
    return torch.softmax(logits.float(), -1).contiguous()
