"""Knowledge distillation from a teacher model or ensemble (Hinton et al. 2015; not in the reference).

An ``ensemble.Ensemble`` of N members costs N forwards per image; distillation takes what it knows back into ONE model: the student is trained
against the teacher's softened probabilities as well as the labels (include/usseg_distill.h has the definition, DESIGN.md section 8 the
gradient).  This module is the loss's owner, with the surface of seg_loss.py's families: ``distill_config`` checks the settings on the host,
``Distill`` holds the teacher, the device settings table and the accumulator, runs the teacher's label-free forward on the current stream and
then the ONE launch of ``ops.distill_loss``.  ``VisionTransformer(loss="distill", distill={...}, teacher=...)`` is the model that calls it.
"""
from __future__ import annotations

import math

import torch

from . import ops
from .seg_loss import SegLoss

DISTILL_KEYS = ("temperature", "soft_weight", "hard_weight")
DISTILL_DEFAULTS = {"temperature": 2.0, "soft_weight": 0.5, "hard_weight": 0.5}
TEMPERATURE_RANGE = (0.125, 8.0)        # the bracket of metrics.fit_temperature


def distill_config(cfg) -> dict:
    """The ``distill`` settings (a dict, or None for every default) -> {"temperature", "soft_weight", "hard_weight"} as Python floats.
    Defaults: temperature 2.0, soft_weight 0.5, hard_weight 0.5 - ordinary choices from the literature; nobody has measured their effect
    on this data.  ValueError for an unknown key, a temperature that is not finite or lies outside [1/8, 8] (the range ``fit_temperature``
    brackets), a weight that is negative or not finite, and both weights zero.  Pure host code."""
    if cfg is not None and not isinstance(cfg, dict):
        raise ValueError(f"distill: a dict of {DISTILL_KEYS} (None or {{}} for the defaults), got {type(cfg).__name__}")
    cfg = dict(cfg or {})
    unknown = [k for k in cfg if k not in DISTILL_KEYS]
    if unknown:
        raise ValueError(f"distill: unknown settings {unknown}; known: {DISTILL_KEYS}")
    try:
        out = {k: float(cfg.get(k, DISTILL_DEFAULTS[k])) for k in DISTILL_KEYS}
    except (TypeError, ValueError) as e:
        raise ValueError(f"distill: every setting is a number: {e}") from None
    T = out["temperature"]
    if not (math.isfinite(T) and TEMPERATURE_RANGE[0] <= T <= TEMPERATURE_RANGE[1]):
        raise ValueError(f"distill: temperature must be finite and lie in [{TEMPERATURE_RANGE[0]}, {TEMPERATURE_RANGE[1]}], got {T}")
    for k in ("soft_weight", "hard_weight"):
        if not (math.isfinite(out[k]) and out[k] >= 0.0):
            raise ValueError(f"distill: {k} must be finite and >= 0, got {out[k]}")
    if out["soft_weight"] == 0.0 and out["hard_weight"] == 0.0:
        raise ValueError("distill: soft_weight and hard_weight are both zero")
    return out


def _table(cfg: dict) -> list:
    return [cfg["temperature"], cfg["soft_weight"], cfg["hard_weight"]] + [0.0] * (ops.DISTILL_SETTINGS - 3)


def teacher_spec(teacher):
    """-> (device, (H, W), input channels, classes, the models inside) of a supported teacher: a ``VisionTransformer`` (the TransUNet variant
    included) or an ``Ensemble`` of such models; ValueError for anything else."""
    from .ensemble import Ensemble
    from .VisionTransformer import VisionTransformer
    if isinstance(teacher, VisionTransformer):
        return teacher.device, tuple(teacher.img_size), int(teacher.input_shape[-1]), int(teacher.num_classes), [teacher]
    if isinstance(teacher, Ensemble):
        return teacher.device, tuple(teacher.img_size), int(teacher.in_channels), int(teacher.num_classes), list(teacher.models)
    raise ValueError(f"distill: the teacher is a VisionTransformer (TBI_TransUNet included) or an Ensemble of them, got {type(teacher).__name__}")


def distill_line(neuralnet):
    """The drivers' extra line of the validation report: the hard and soft terms of the LAST validation batch when the model trains with
    ``loss="distill"`` (one read-back per epoch), else None (nothing is printed)."""
    terms = getattr(neuralnet, "distill_terms", None)
    terms = None if terms is None else terms()
    return None if terms is None else "hard = {}, soft = {}".format(terms["hard"], terms["soft"])


def load_teacher(checkpoints, img_size, in_channels, device, *, num_classes=3, use_vit=False, transunet=False, flip=False):
    """The drivers' ``teacher=`` from checkpoint paths (one path, a comma-separated string or a list): each loads into a model of the
    student's geometry through ``load`` (the loader the evaluator's ``--bleed`` uses); more than one checkpoint, or ``flip``, makes an
    ``Ensemble``."""
    from .ensemble import Ensemble
    paths = [p for p in checkpoints.split(",") if p] if isinstance(checkpoints, str) else list(checkpoints)
    if not paths:
        raise ValueError("distill: no teacher checkpoint given")
    models = []
    for path in paths:
        if transunet:
            from .TBI_TransUNet import VisionTransformer as Model
            m = Model(img_size=tuple(img_size), num_classes=num_classes, in_channels=in_channels, device=str(device))
        else:
            from .VisionTransformer import VisionTransformer as Model
            m = Model(1, img_size=tuple(img_size), num_classes=num_classes, in_channels=in_channels, use_vit=use_vit, device=str(device))
        m.load(path)
        models.append(m)
    return Ensemble(models, flip=flip) if len(models) > 1 or flip else models[0]


class Distill(SegLoss):
    """``Distill(teacher, config, student)``: the distillation loss of ``student`` (a ``VisionTransformer``) against ``teacher``; without
    ``student`` only the settings are checked (``seg_loss.resolve``), and ``place(student)`` does the rest once the student has its device.

    Owns the teacher, the device settings table (``settings``: temperature, soft_weight, hard_weight - read by the kernel when it runs, so a
    captured graph follows ``set_distill`` on its next replay) and the accumulator (``acc``: [0] the loss).  The teacher is never trained: only its
    label-free ``_predict_body`` runs, which reads no loss buffer, gradient, optimiser state or BatchNorm statistic and writes none.

    Refused with a ValueError: a teacher that is (or contains) the student, a teacher on another device or with another image size, input
    channel or class count, and a teacher whose ``_predict_state()`` is not empty (Arch A members with their always-on dropout: a captured
    training step would have to carry their counters)."""

    acc_floats = ops.DISTILL_ACC_FLOATS
    reported = 4            # ``compute_loss`` has no input that could show a teacher: the HARD term alone, weighted

    def __init__(self, teacher, config, student=None):
        self.config = distill_config(config)
        self.teacher = teacher
        if student is not None:
            self.place(student)

    def place(self, student):
        teacher = self.teacher
        dev, hw, cin, ncls, models = teacher_spec(teacher)
        if any(m is student for m in models) or teacher is student:
            raise ValueError("distill: the teacher is the student itself")
        own = (student.device, tuple(student.img_size), int(student.input_shape[-1]), int(student.num_classes))
        for what, a, b in zip(("device", "image size", "input channels", "class count"), (dev, hw, cin, ncls), own):
            if a != b:
                raise ValueError(f"distill: the teacher's {what} is {a}, the student's {b}")
        if teacher._predict_state():
            raise ValueError("distill: a teacher whose predict advances device state (TBI_ResNest.ResNest members with their always-on dropout) "
                             "is out of scope: a captured training step would have to carry its counters")
        super().place(student)
        self.settings = torch.tensor(_table(self.config), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ the settings on the device
    def distill_settings(self) -> dict:
        """The settings the next step uses, read from the device (synchronises)."""
        v = self.settings.tolist()
        return {"temperature": v[0], "soft_weight": v[1], "hard_weight": v[2]}

    def set_distill(self, temperature=None, soft_weight=None, hard_weight=None):
        """From the next step on, eager or replayed: the kernel reads the device table, so a captured graph needs no recapture.  A setting left
        None keeps its value; the combination passes ``distill_config``."""
        given = {k: v for k, v in (("temperature", temperature), ("soft_weight", soft_weight), ("hard_weight", hard_weight)) if v is not None}
        self.config = distill_config({**self.config, **given})
        self.settings.copy_(torch.tensor(_table(self.config), dtype=torch.float32))

    def state(self):
        return {"__distill__": self.settings.detach().clone()}

    def load_state(self, d):
        """A checkpoint's table (fp32 [DISTILL_SETTINGS]) -> the device, checked like ``set_distill``."""
        t = d.get("__distill__")
        super().load_state(d)                   # (pops every family's entry; this one's is no plain copy)
        if t is not None:
            self.set_distill(*(float(a) for a in t.tolist()[:3]))

    def distill_terms(self) -> dict:
        """{"hard", "soft"}: the two weighted terms of the LAST call (their sum is the loss); synchronises."""
        v = self.acc[4:6].tolist()
        return {"hard": v[0], "soft": v[1]}

    # ------------------------------------------------------------------ the step's part
    def teacher_probs(self, x):
        """The teacher's probabilities on the CURRENT stream (no new stream or event): fp32 [B,H,W,C]; an ``Ensemble``'s are the mean of its members."""
        q = self.teacher._predict_body(x)
        q = getattr(q, "probs", q)
        return q if q.is_contiguous() else q.contiguous()

    def loss_into(self, acc, x, probs, y, dlogits, *, scale, ov_scale=1.0, quad_w=0):
        """``teacher._predict_body(x)`` on the current stream, then the ONE launch: the scalar loss in ``acc[0]``, ``dlogits`` written when given.
        ``x`` None (``compute_loss``): the teacher's place is taken by ``probs`` itself, q == p, whose soft term is exactly zero."""
        _, H, W, C = probs.shape
        q = probs if x is None else self.teacher_probs(x)
        ops.distill_loss(probs, y, q, self.settings, acc, dlogits, HW=H * W, C_classes=C, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=scale,
                         quad_w=quad_w)
