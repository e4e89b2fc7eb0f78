"""The segmentation losses of ``VisionTransformer``, one owner per family.  ``resolve`` picks it on the host (every refusal); the model calls ``place`` once it has a device, then only
  * ``acc``: the accumulator whose [0] is the scalar loss (the model's ``_loss``: one tensor for the model's life, a captured graph holds it);
  * ``fused_head``: the loss runs INSIDE the model's head + softmax + loss launch (``PixelLoss`` alone); every other owner is handed the probabilities;
  * ``loss_into(acc, x, probs, y, dlogits, *, scale, ov_scale, quad_w)``: the family's launches - the scalar loss into ``acc[0]``, ``dlogits`` when given;
  * ``state()`` / ``load_state(d)`` (the checkpoint entries) and what the model's public properties and setters hand on.
"""
from __future__ import annotations

import math

import torch

from . import ops

LOSSES = ("cce", "my_loss_cat", "focal")             # the reference's own: per-pixel losses inside the fused head launch
OVERLAP_LOSSES = ("dice", "tversky", "dice_ce")      # region-overlap losses (not in the reference): two launches behind the probabilities-only head
LOVASZ_LOSSES = ("lovasz", "lovasz_ce")              # the Lovasz-softmax loss (not in the reference): a device sort of the pixel errors behind that head
TOPK_LOSSES = ("topk", "dice_topk")                  # the top-k (hard-pixel) cross-entropy (not in the reference): a device radix select behind that head
DISTILL_LOSSES = ("distill",)                        # knowledge distillation from a teacher (not in the reference): distill.Distill owns it, one launch behind that head
STATE_KEYS = ("__boundary_weight__", "__topk_fraction__", "__distill__")      # every family's checkpoint entries
_CCE = dict(label_smoothing=0.1, clip_eps=1e-7)      # the reference's CategoricalCrossentropy (:205), inside every family


def overlap_settings(loss, overlap):
    """What the drivers hand the constructor: for a region-overlap loss with no settings given, the empty dict (every default)."""
    return {} if overlap is None and loss in OVERLAP_LOSSES else overlap


def overlap_config(loss, num_classes, overlap):
    """``loss`` in OVERLAP_LOSSES and the ``overlap`` settings (dict or None) -> ``ops.overlap_loss(...)``; ValueError for a bad or
    contradictory combination."""
    cfg = dict(overlap or {})
    unknown = [k for k in cfg if k not in ops.OVERLAP_KEYS]
    if unknown:
        raise ValueError(f"overlap: unknown settings {unknown}; known: {ops.OVERLAP_KEYS}")
    if loss != "tversky" and ("alpha" in cfg or "beta" in cfg):
        raise ValueError(f"overlap: alpha / beta belong to loss='tversky'; '{loss}' is alpha = beta = 0.5")
    if loss != "dice_ce" and cfg.get("ce_weight", 0.0) != 0.0:
        raise ValueError(f"overlap: a cross-entropy term needs loss='dice_ce', not '{loss}'")
    if loss == "dice_ce" and cfg.get("ce_weight", 1.0) == 0.0:
        raise ValueError("overlap: loss='dice_ce' with ce_weight = 0 is loss='dice'")
    w = cfg.get("class_weight")
    w = [1.0 / num_classes] * num_classes if w is None else [float(v) for v in w]
    if len(w) != num_classes:
        raise ValueError(f"overlap: class_weight has {len(w)} entries for {num_classes} classes")
    a, b = (0.3, 0.7) if loss == "tversky" else (0.5, 0.5)
    return ops.overlap_loss(w, cfg.get("alpha", a), cfg.get("beta", b), cfg.get("smooth", 1.0), cfg.get("power", 1.0), cfg.get("ov_weight", 1.0),
                            cfg.get("ce_weight", 1.0 if loss == "dice_ce" else 0.0))


def lovasz_config(loss, num_classes, lovasz):
    """``loss`` in LOVASZ_LOSSES and the ``lovasz`` settings (dict or None: every default) -> ``ops.lovasz_loss(...)``; ValueError for a bad or
    contradictory combination."""
    if lovasz is not None and not isinstance(lovasz, dict):
        raise ValueError(f"lovasz: a dict of {ops.LOVASZ_KEYS} (None or {{}} for the defaults), got {type(lovasz).__name__}")
    cfg = dict(lovasz or {})
    unknown = [k for k in cfg if k not in ops.LOVASZ_KEYS]
    if unknown:
        raise ValueError(f"lovasz: unknown settings {unknown}; known: {ops.LOVASZ_KEYS}")
    if loss != "lovasz_ce" and cfg.get("ce_weight", 0.0) != 0.0:
        raise ValueError(f"lovasz: a cross-entropy term needs loss='lovasz_ce', not '{loss}'")
    if loss == "lovasz_ce" and cfg.get("ce_weight", 1.0) == 0.0:
        raise ValueError("lovasz: loss='lovasz_ce' with ce_weight = 0 is loss='lovasz'")
    w = cfg.get("class_weight")
    w = [1.0] * num_classes if w is None else [float(v) for v in w]
    if len(w) != num_classes:
        raise ValueError(f"lovasz: class_weight has {len(w)} entries for {num_classes} classes")
    return ops.lovasz_loss(w, cfg.get("lv_weight", 1.0), cfg.get("ce_weight", 1.0 if loss == "lovasz_ce" else 0.0), cfg.get("threshold", 0.5),
                           cfg.get("classes", "present"))


def topk_config(loss, num_classes, topk, *, overlap=None, class_factor=None, focal_gamma=None, boundary=None, lovasz=None):
    """``loss`` in TOPK_LOSSES and the ``topk`` settings (dict or None: every default) -> (``ops.topk_loss(...)``, the fraction, the Dice term's
    ``ops.overlap_loss(...)`` for "dice_topk" or None); ValueError for a bad or contradictory combination."""
    if loss not in TOPK_LOSSES:
        raise ValueError(f"topk settings only apply to loss in {TOPK_LOSSES}")
    if topk is not None and not isinstance(topk, dict):
        raise ValueError(f"topk: a dict of {ops.TOPK_KEYS} (None or {{}} for the defaults), got {type(topk).__name__}")
    cfg = dict(topk or {})
    unknown = [k for k in cfg if k not in ops.TOPK_KEYS]
    if unknown:
        raise ValueError(f"topk: unknown settings {unknown}; known: {ops.TOPK_KEYS}")
    if class_factor is not None or focal_gamma is not None:
        raise ValueError(f"class_factor / focal_gamma do not apply to loss='{loss}'")
    if boundary is not None or lovasz is not None:
        raise ValueError(f"boundary / lovasz settings do not combine with loss='{loss}'")
    ov = None
    if loss == "topk":
        if overlap is not None:
            raise ValueError("overlap settings need loss='dice_topk', not 'topk'")
    else:
        if dict(overlap or {}).get("ce_weight", 0.0) != 0.0:
            raise ValueError("overlap: the cross-entropy of loss='dice_topk' is its top-k term; ce_weight must be 0")
        ov = overlap_config("dice", num_classes, overlap)
    fraction = ops.topk_fraction_value(cfg.get("fraction", 0.1))
    return ops.topk_loss(cfg.get("tk_weight", 1.0), cfg.get("scope", "batch")), fraction, ov


def boundary_config(loss, num_classes, boundary):
    """The ``boundary`` settings (dict) of a model with ``loss`` in OVERLAP_LOSSES -> (weight, ``ops.boundary_loss(...)``, threshold); ValueError for
    any other loss, an unknown key, a negative or non-finite weight, a wrong-length ``class_weight`` or a NaN threshold."""
    if loss not in OVERLAP_LOSSES:
        raise ValueError(f"boundary: the boundary term is an add-on to loss in {OVERLAP_LOSSES}, not to '{loss}'")
    if not isinstance(boundary, dict):
        raise ValueError(f"boundary: a dict of {ops.BOUNDARY_KEYS} ({{}} for the defaults), got {type(boundary).__name__}")
    unknown = [k for k in boundary if k not in ops.BOUNDARY_KEYS]
    if unknown:
        raise ValueError(f"boundary: unknown settings {unknown}; known: {ops.BOUNDARY_KEYS}")
    weight = _boundary_weight(boundary.get("weight", 0.01))
    u = boundary.get("class_weight")
    u = [0.0] + [1.0] * (num_classes - 1) if u is None else [float(v) for v in u]
    if len(u) != num_classes:
        raise ValueError(f"boundary: class_weight has {len(u)} entries for {num_classes} classes")
    thr = float(boundary.get("threshold", 0.5))
    if math.isnan(thr):
        raise ValueError("boundary: threshold is NaN")
    return weight, ops.boundary_loss(u), thr


def _boundary_weight(w):
    w = float(w)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"boundary: weight must be finite and >= 0, got {w}")
    return w


class SegLoss:
    """What the model asks of every owner, with the answers of a family that has no such part."""
    fused_head, acc_floats = False, ops.OVERLAP_ACC_FLOATS
    reported = 0                                     # the float of a fresh accumulator that ``compute_loss`` returns
    alpha, class_factor = 2, None                    # the reference's attributes (:208-209): the focal exponent; ``resolve`` sets the class factors
    overlap = lovasz = topk = boundary = None        # the family's descriptor: the model's ``overlap_loss``, ``lovasz_loss``, ``topk_loss``, ``boundary_loss``
    saved = {}                                       # checkpoint key -> the device tensor behind it
    boundary_weight = topk_fraction = distill_settings = distill_terms = lambda self: None      # (a family that has the setting reads it from the device)

    def place(self, model):
        self.device = model.device
        self.acc = torch.zeros(self.acc_floats, dtype=torch.float32, device=self.device)      # [0] = the scalar loss

    def state(self):
        return {k: t.detach().clone() for k, t in self.saved.items()}

    def load_state(self, d):
        """Pops EVERY family's entries from ``d`` (another family's is ignored); a checkpoint without this family's leaves the constructor's value."""
        for k, v in [(k, d.pop(k)) for k in STATE_KEYS if k in d]:
            if k in self.saved:
                self.saved[k].copy_(v.to(self.device))

    def set_boundary_weight(self, w):
        raise ValueError("set_boundary_weight: the model was built without boundary=")

    def set_topk_fraction(self, f):
        raise ValueError(f"set_topk_fraction: the model was built without loss in {TOPK_LOSSES}")

    def set_distill(self, temperature=None, soft_weight=None, hard_weight=None):
        raise ValueError(f"set_distill: the model was built without loss in {DISTILL_LOSSES}")


class PixelLoss(SegLoss):
    """"cce", "my_loss_cat", "focal" (``class_loss``: None for the first): the step's loss runs in the model's head launch, ``loss_into`` serves ``compute_loss``."""
    fused_head, acc_floats = True, ops.ACC_FLOATS

    def __init__(self, class_loss):
        self.class_loss = class_loss

    def loss_into(self, acc, x, probs, y, dlogits, *, scale, ov_scale, quad_w):
        assert dlogits is None, "the gradient of a per-pixel loss comes from the model's head launch"
        _, H, W, C = probs.shape
        ops.loss_from_probs(probs, y, acc, HW=H * W, C_classes=C, loss_kind=0, inv_global_batch=scale, class_loss=self.class_loss, **_CCE)


class OverlapLoss(SegLoss):
    """"dice", "tversky", "dice_ce": the sums pass (scalar loss and backward coefficients into ``acc``), then the backward pass.  ``bnd`` (``boundary_config``'s
    result, or None) adds the boundary term: its weight lives on the device (``wb``), the labels' distance map is computed once per call."""

    def __init__(self, overlap, bnd=None):
        self.overlap, self.wb = overlap, None
        self.weight0, self.boundary, self.threshold = bnd or (None, None, 0.5)

    def place(self, model):
        super().place(model)
        if self.boundary is not None:
            self.wb = torch.full((1,), self.weight0, dtype=torch.float32, device=self.device)      # read by the sums kernel when it runs
            self.saved = {"__boundary_weight__": self.wb}

    def loss_into(self, acc, x, probs, y, dlogits, *, scale, ov_scale, quad_w):
        _, H, W, C = probs.shape
        kw = dict(overlap=self.overlap, HW=H * W, C_classes=C, inv_global_batch=scale, **_CCE)
        if self.boundary is not None:           # the labels' distance map once per step, then the pair that carries the boundary term
            phi = ops.sdf_labels(y, threshold=self.threshold)
            ops.overlap_boundary_loss_sums(probs, y, phi, acc, boundary=self.boundary, wb=self.wb, ov_scale=ov_scale, **kw)
            if dlogits is not None:
                ops.overlap_boundary_loss_bwd(probs, y, phi, acc, dlogits, boundary=self.boundary, quad_w=quad_w, **kw)
            return
        ops.overlap_loss_sums(probs, y, acc, ov_scale=ov_scale, **kw)
        if dlogits is not None:
            ops.overlap_loss_bwd(probs, y, acc, dlogits, quad_w=quad_w, **kw)

    def boundary_weight(self):
        return None if self.wb is None else float(self.wb.item())

    def set_boundary_weight(self, w):
        if self.wb is None:
            super().set_boundary_weight(w)
        self.wb.fill_(_boundary_weight(w))


class LovaszLoss(SegLoss):
    """"lovasz", "lovasz_ce": the coefficients pass (device sort), the sums pass (scalar loss and k_c into ``acc``), then the backward pass."""

    def __init__(self, lovasz):
        self.lovasz = lovasz
        self.bufs = {}                          # (pixels of a call, classes) -> (g, counts, workspace): allocated once per model and batch shape

    def loss_into(self, acc, x, probs, y, dlogits, *, scale, ov_scale, quad_w):
        B, H, W, C = probs.shape
        M = B * H * W
        if (M, C) not in self.bufs:
            self.bufs[(M, C)] = (torch.empty(max(M * C, 4), dtype=torch.float32, device=self.device), torch.zeros(4, dtype=torch.int32, device=self.device),
                                 torch.empty(max(ops.lovasz_ws_bytes(M, C), 16), dtype=torch.uint8, device=self.device))
        g, counts, ws = self.bufs[(M, C)]
        g = g[:M * C].view(probs.shape)
        kw = dict(lovasz=self.lovasz, HW=H * W, C_classes=C)
        ops.lovasz_coeffs(probs, y, g, counts, ws, **kw)
        kw.update(inv_global_batch=scale, **_CCE)
        ops.lovasz_loss_sums(probs, y, g, counts, acc, ov_scale=ov_scale, **kw)
        if dlogits is not None:
            ops.lovasz_loss_bwd(probs, y, g, acc, dlogits, quad_w=quad_w, **kw)


class TopkLoss(SegLoss):
    """"topk", "dice_topk": the per-pixel losses with their exact selection, the sums pass (scalar loss and coefficient into ``acc``), then the backward
    pass.  ``dice`` is the Dice half of "dice_topk" (or None): its sums go to an accumulator of their own (``ov_acc``) between the two."""

    def __init__(self, topk, fraction, dice=None):
        self.topk, self.fraction0, self.dice = topk, fraction, dice
        self.bufs = {}                          # (pixels of a call, pixels of an image) -> workspace: allocated once per model and batch shape

    def place(self, model):
        super().place(model)
        self.fraction = torch.full((1,), self.fraction0, dtype=torch.float32, device=self.device)      # read by the select kernels when they run
        self.saved = {"__topk_fraction__": self.fraction}
        self.ov_acc = None if self.dice is None else torch.zeros_like(self.acc)

    def loss_into(self, acc, x, probs, y, dlogits, *, scale, ov_scale, quad_w):
        B, H, W, C = probs.shape
        key = (B * H * W, H * W)
        if key not in self.bufs:
            self.bufs[key] = torch.empty(max(ops.topk_ws_bytes(*key, ops.TOPK_SCOPES[self.topk.scope]), 16), dtype=torch.uint8, device=self.device)
        ws = self.bufs[key]
        ov_acc = self.ov_acc if acc is self.acc or self.dice is None else torch.zeros_like(acc)      # (a foreign accumulator: a Dice one of its own)
        kw = dict(topk=self.topk, HW=H * W, C_classes=C, **_CCE)
        ops.topk_pixel_loss(probs, y, self.fraction, ws, **kw)
        kw.update(inv_global_batch=scale, overlap_acc=ov_acc)
        if ov_acc is not None:
            ops.overlap_loss_sums(probs, y, ov_acc, overlap=self.dice, HW=H * W, C_classes=C, ov_scale=ov_scale, inv_global_batch=scale, **_CCE)
        ops.topk_loss_sums(probs, ws, acc, **kw)
        if dlogits is not None:
            ops.topk_loss_bwd(probs, y, ws, acc, dlogits, quad_w=quad_w, **kw)

    def topk_fraction(self):
        return float(self.fraction.item())

    def set_topk_fraction(self, f):
        self.fraction.fill_(ops.topk_fraction_value(f))


def resolve(loss, num_classes, *, class_factor=None, focal_gamma=None, overlap=None, alpha=None, beta=None, smooth=None, power=None, class_weight=None,
            ce_weight=None, ov_weight=None, boundary=None, lovasz=None, topk=None, distill=None, teacher=None):
    """The constructor's loss keywords -> the owner of ``loss``, not yet placed; ValueError for every bad or contradictory combination.  Pure host code."""
    from .distill import Distill                # (that module imports this one)
    if loss not in LOSSES + OVERLAP_LOSSES + LOVASZ_LOSSES + TOPK_LOSSES + DISTILL_LOSSES:
        raise ValueError(f"loss must be one of {LOSSES + OVERLAP_LOSSES + LOVASZ_LOSSES + TOPK_LOSSES + DISTILL_LOSSES}, got {loss!r}")
    owner = None
    if loss in DISTILL_LOSSES:
        if teacher is None:
            raise ValueError(f"loss='{loss}' needs teacher=: a VisionTransformer or an Ensemble of them")
        given_other = dict(class_factor=class_factor, focal_gamma=focal_gamma, overlap=overlap, boundary=boundary, lovasz=lovasz, topk=topk, alpha=alpha,
                           beta=beta, smooth=smooth, power=power, class_weight=class_weight, ce_weight=ce_weight, ov_weight=ov_weight)
        other = [k for k, v in given_other.items() if v is not None]
        if other:
            raise ValueError(f"{other} do not combine with loss='{loss}' (its settings are distill={{...}})")
        owner = Distill(teacher, distill)       # (its settings are refused here, before anything is built)
    elif distill is not None or teacher is not None:
        raise ValueError(f"distill= / teacher= only apply to loss in {DISTILL_LOSSES}, not to '{loss}'")
    if lovasz is not None and loss not in LOVASZ_LOSSES:
        raise ValueError(f"lovasz settings only apply to loss in {LOVASZ_LOSSES}")
    if loss in LOVASZ_LOSSES and (class_factor is not None or focal_gamma is not None):
        raise ValueError(f"class_factor / focal_gamma do not apply to loss='{loss}' (its weights are lovasz['class_weight'])")
    if loss in LOVASZ_LOSSES:
        owner = LovaszLoss(lovasz_config(loss, num_classes, lovasz))
    given = dict(alpha=alpha, beta=beta, smooth=smooth, power=power, class_weight=class_weight, ce_weight=ce_weight, ov_weight=ov_weight)
    overlap_kw = {k: v for k, v in given.items() if v is not None}      # (the keyword ``alpha`` is Tversky's; the owner's ``alpha`` below is the focal exponent, :208)
    if overlap is not None and overlap_kw:
        raise ValueError("give the overlap settings as overlap={...} or as keywords, not both")
    overlap = overlap if overlap is not None else (overlap_kw or None)
    if topk is not None or loss in TOPK_LOSSES:
        owner = TopkLoss(*topk_config(loss, num_classes, topk, overlap=overlap, class_factor=class_factor, focal_gamma=focal_gamma, boundary=boundary, lovasz=lovasz))
        overlap = None                          # (the Dice term of "dice_topk" is held apart: the overlap pair itself does not run the step)
    if overlap is not None and loss not in OVERLAP_LOSSES:
        raise ValueError(f"overlap settings only apply to loss in {OVERLAP_LOSSES}")
    if loss in OVERLAP_LOSSES and overlap is None:
        raise ValueError(f"loss={loss!r} needs its settings: overlap={{}} for the defaults, or any of {ops.OVERLAP_KEYS}")
    if loss in OVERLAP_LOSSES and (class_factor is not None or focal_gamma is not None):
        raise ValueError(f"class_factor / focal_gamma do not apply to loss='{loss}' (its weights are overlap['class_weight'])")
    ov = overlap_config(loss, num_classes, overlap) if loss in OVERLAP_LOSSES else None
    bnd = None if boundary is None else boundary_config(loss, num_classes, boundary)
    if focal_gamma is not None and loss != "focal":
        raise ValueError("focal_gamma only applies to loss='focal'")
    factor = [0.06329, 0.027567, 0.90914] if class_factor is None else [float(v) for v in class_factor]   # :209
    if (loss == "my_loss_cat" or class_factor is not None) and len(factor) != num_classes:
        raise ValueError(f"class_factor has {len(factor)} entries for {num_classes} classes")
    if loss == "my_loss_cat":
        owner = PixelLoss(ops.class_loss(factor, 0.0, 3.0))                         # :270
    elif loss == "focal":
        gamma = float(SegLoss.alpha if focal_gamma is None else focal_gamma)
        weighted = class_factor is not None
        owner = PixelLoss(ops.class_loss(factor if weighted else [1.0] * num_classes, gamma, 3.0 if weighted else 1.0))   # :272-273,277
    elif ov is not None:
        owner = OverlapLoss(ov, bnd)
    owner = owner or PixelLoss(None)            # "cce"
    owner.class_factor = factor
    return owner
