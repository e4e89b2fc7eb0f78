"""A float64 torch restatement of the reference's second Arch B loss, ``VisionTransformer.my_loss_cat`` (VisionTransformer.py:259-280), and
of the focal line it keeps commented (:272-273), written line by line after the reference - not after the kernels.

One parametrised family ("class loss") covers both forms.  Per pixel, probabilities p[c], labels y[c], C classes:

    ys[c] = y[c]*0.9 + 0.1/C                                  (:262-263; on a copy - the reference smooths its own tensor)
    pc[c] = clip(p[c], 1e-7, 1 - 1e-7)                        (:266; NOT divided by the class sum)
    l     = -factor * sum_c w[c] * ys[c] * (1 - pc[c])^gamma * log(pc[c])
    map[h,w] = sum_b l[b,h,w]                                 (:270, axis=[0,3]: what my_loss_cat returns)
    scalar   = sum_{h,w} map / global_batch                   (compute_loss, :225-227)

  * my_loss_cat as committed (:270): factor 3, w = class_factor (:209), gamma 0;
  * the focal line (:272-273, and :277 "-3 if using class factor, -1 otherwise"): factor 1, w = 1, gamma = alpha = 2 (:208).

The reference clips an fp32 tensor, so the two clip constants are the fp32 values of 1e-7 and of 1 - 1e-7 (= 1 - 2^-23).
"""
import numpy as np
import torch

CLASS_FACTOR = [0.06329, 0.027567, 0.90914]     # VisionTransformer.py:209
ALPHA = 2                                       # :208
LO = float(np.float32(1e-7))                    # tf.clip_by_value(y_pred, 1e-7, 1. - 1e-7) on an fp32 tensor (:266)
HI = float(np.float32(1.0 - 1e-7))
SMOOTH = 0.1

# (w, gamma, factor) of the forms the tests run
FORMS = {
    "my_loss_cat": (CLASS_FACTOR, 0.0, 3.0),          # :270, as committed
    "focal": ([1.0, 1.0, 1.0], float(ALPHA), 1.0),    # :272-273
    "weighted_focal": (CLASS_FACTOR, 1.5, 3.0),       # class factors and a focal exponent together, factor 3 (:277)
}


def form(name, C=3):
    """(w, gamma, factor) of a named form for C classes: the reference's three class factors, cycled / cut to C."""
    w, gamma, factor = FORMS[name]
    return [w[c % len(w)] for c in range(C)], gamma, factor


def flat_inputs(C=3, B=2, H=9, W=11, seed=1234):
    """The inputs of the kernel tests: fp32-representable logits 3*randn [B,H,W,C] with one row forced to [40, -40, 0, 0][:C] (reaches both
    clip constants by many orders of magnitude), and soft labels."""
    gen = torch.Generator().manual_seed(seed + C)
    logits = (torch.randn(B, H, W, C, generator=gen, dtype=torch.float64) * 3).float().double()
    logits[0, 0, 0] = torch.tensor([40.0, -40.0, 0.0, 0.0][:C], dtype=torch.float64)
    y = torch.softmax(2 * torch.randn(B, H, W, C, generator=gen, dtype=torch.float64), -1).float().double()
    return logits, y


def per_pixel(y_true, y_pred, w, gamma, factor):
    """l [B,H,W] in float64.  ``gamma == 0`` takes the reference's committed line (no pow at all); any other gamma its focal line with the weights."""
    y_true = y_true.double().clone()                 # the reference's `y_true *= 0.9` acts on the tensor tf.function handed it; the caller's stays
    y_pred = y_pred.double()
    C = y_pred.shape[-1]
    y_true *= 1.0 - SMOOTH                                                                   # :262
    y_true += SMOOTH / C                                                                     # :263
    y_pred = torch.clamp(y_pred, LO, HI)                                                     # :266
    cf = torch.as_tensor(w, dtype=torch.float64, device=y_pred.device)
    if gamma == 0:
        return -factor * torch.sum(y_true * torch.log(y_pred) * cf, dim=-1)                  # :270 (axis 3)
    return -factor * torch.sum(y_true * torch.log(y_pred) * torch.pow(1.0 - y_pred, gamma) * cf, dim=-1)   # :272-273 (axis 3)


def loss_map(y_true, y_pred, w, gamma, factor):
    """my_loss_cat's return value: [H,W], summed over the batch too (:270, axis=[0,3])."""
    return per_pixel(y_true, y_pred, w, gamma, factor).sum(0)


def scalar(y_true, y_pred, w, gamma, factor, global_batch):
    """compute_loss with this loss (:225-227): compute_average_loss sums everything and divides by the GLOBAL batch."""
    return loss_map(y_true, y_pred, w, gamma, factor).sum() / global_batch


def my_loss_cat(y_true, y_pred):
    """The public method as committed."""
    return loss_map(y_true, y_pred, *FORMS["my_loss_cat"])


def from_logits(logits, y_true, w, gamma, factor, inv_scale):
    """softmax -> loss, as the kernels run it.  logits fp64 [..., C].  -> dict: probs, loss (= inv_scale * sum of l), dlogits (autograd),
    dLdp (autograd at the probabilities), mag (the magnitude of the dlogits bound), edge (pixels with a probability within 2^-20 relative of a
    clip constant: fp32 arithmetic may clip there where fp64 does not)."""
    z = logits.double().clone().requires_grad_(True)
    p = torch.softmax(z, -1)
    p.retain_grad()
    loss = per_pixel(y_true, p, w, gamma, factor).sum() * inv_scale
    loss.backward()
    pd, dLdp = p.detach(), p.grad
    # d loss / d z[k] = p[k]*(dLdp[k] - sum_c dLdp[c]*p[c]): what its terms can add up to in magnitude
    mag = pd * (dLdp.abs() + (dLdp.abs() * pd).sum(-1, keepdim=True))
    rel = 2.0 ** -20
    edge = (((pd - LO).abs() <= rel * LO) | ((pd - HI).abs() <= rel * HI)).any(-1)
    return dict(probs=pd, loss=loss.detach(), dlogits=z.grad, dLdp=dLdp, mag=mag, edge=edge)
