"""Ensemble prediction with uncertainty maps (not in the reference).

``Ensemble(models, flip=False, draws=1)`` runs every member's own ``_predict_body`` on one input and merges the member probabilities in ONE
launch (``ops.ensemble_merge`` -> ``usseg_ensemble_merge``, csrc/ensemble.hip):

    members   for each model, for each view in (identity, left-right mirrored if ``flip``), for each draw in range(draws) - in that order;
    probs     the fp32 mean of the members, added in member order (a mirrored member is un-mirrored as it is read);
    entropy   the predictive entropy H of the mean;  mutual_info  H minus the mean member entropy (the BALD term): what the members
              disagree about;  variance  the per-class variance over the members;
    image_scores / image_counts   four numbers per image (``ops.ensemble_image_scores``).

Three uses.  Several checkpoints: a deep ensemble.  ``flip=True``: the test-time augmentation that matches the left-right flip
``TBI_TransUNet.dataAug`` trains with.  ``draws > 1`` on Arch A (``TBI_ResNest.ResNest``): Monte-Carlo dropout - its ``predict`` keeps the
reference's always-on dropout and draws fresh masks from a device counter on every call, so each draw is one more sample and the counter
advances by ``draws`` per ensemble call.  An Arch B model is deterministic in ``predict``; repeating it adds nothing and is refused.

``Ensemble`` is a ``step.PredictDriver``: ``predict`` runs eagerly or replays ONE captured HIP graph that holds every member and the merge
(``capture_predict_graph``; its warm-up gives the dropout draws back, as for a single Arch A model).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops
from ._lib import ENSEMBLE_MAX
from .step import PredictDriver
from .TBI_ResNest import ResNest
from .VisionTransformer import VisionTransformer


class EnsembleOutput(NamedTuple):
    probs: torch.Tensor                   # fp32 [B,H,W,C]: the mean of the members
    entropy: torch.Tensor                 # fp32 [B,H,W]: the predictive entropy of the mean
    mutual_info: torch.Tensor             # fp32 [B,H,W]: the entropy of the mean minus the mean member entropy, >= 0
    variance: Optional[torch.Tensor]      # fp32 [B,H,W,C]: the variance over the members
    image_scores: torch.Tensor            # fp32 [B,4]: mean entropy, mean / max mutual information, mean entropy where the last class wins
    image_counts: torch.Tensor            # int32 [B]: the pixels where the last class wins


def _spec(m):
    """-> (device, (H, W), input channels, classes, random in predict) of a supported model."""
    if isinstance(m, VisionTransformer):
        return m.device, tuple(m.img_size), int(m.input_shape[-1]), int(m.num_classes), False
    if isinstance(m, ResNest):
        return m.device, (int(m.height), int(m.width)), int(m.channel), int(m.num_class), True
    raise ValueError(f"Ensemble takes VisionTransformer (TBI_TransUNet included) or TBI_ResNest.ResNest models, got {type(m).__name__}")


class Ensemble(PredictDriver):
    """``Ensemble(models, flip=False, draws=1)``: see the module docstring.  ``predict(x)`` takes x [B,H,W,C] (numpy or tensor) and returns an
    ``EnsembleOutput``; after ``capture_predict_graph`` it holds the graph's static buffers (valid until the next call)."""

    def __init__(self, models, *, flip=False, draws=1):
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not models:
            raise ValueError("Ensemble needs at least one model")
        specs = [_spec(m) for m in models]
        for s in specs[1:]:
            for what, a, b in zip(("devices", "image sizes", "input channels", "class counts"), specs[0][:4], s[:4]):
                if a != b:
                    raise ValueError(f"the models' {what} differ: {a} and {b}")
        draws = int(draws)
        if draws < 1:
            raise ValueError(f"draws must be >= 1, got {draws}")
        if draws > 1 and not all(s[4] for s in specs):
            raise ValueError("draws > 1 needs models whose predict is random (TBI_ResNest.ResNest): identical passes add nothing")
        self.models, self.flip, self.draws = models, bool(flip), draws
        self.members = len(models) * (2 if self.flip else 1) * draws
        if self.members > ENSEMBLE_MAX:
            raise ValueError(f"{self.members} members (models x views x draws) exceed the {ENSEMBLE_MAX} one merge launch takes")
        self.device, self.img_size, self.in_channels, self.num_classes = specs[0][:4]
        self.input_shape = [self.img_size[0], self.img_size[1], self.in_channels]

    # ------------------------------------------------------------------ PredictDriver hooks
    def _prep_x(self, x):
        x = self.models[0]._prep_x(x)
        H, W = self.img_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (H, W, self.in_channels):
            raise ValueError(f"expected input [B,{H},{W},{self.in_channels}], got {tuple(x.shape)}")
        return x

    def _predict_state(self):
        return [t for m in self.models for t in m._predict_state()]

    def _predict_body(self, x):
        """Every member on the current stream in the fixed member order, then one merge and one image-scores launch; no host synchronisation.
        ``x`` is what the members' ``_predict_body`` takes ([B,H,W,*]: the mirror runs along W)."""
        xm = torch.flip(x, dims=(2,)) if self.flip else None        # once, shared by the models (plumbing: one copy of the input)
        members, flip_w = [], 0
        for m in self.models:
            for mirrored in ((False, True) if self.flip else (False,)):
                for _ in range(self.draws):
                    if mirrored:
                        flip_w |= 1 << len(members)
                    members.append(m._predict_body(xm if mirrored else x))
        probs, entropy, mutual_info, variance = ops.ensemble_merge(members, flip_w)
        scores, counts = ops.ensemble_image_scores(probs, entropy, mutual_info)
        return EnsembleOutput(probs, entropy, mutual_info, variance, scores, counts)
