"""The model computation of the reference's inference driver ``TBIEvaluator.py`` (``Polar_Model`` / ``PolarProcess``, duplicated in
``DisplayInference.py``) with ``use_brainMask=True``: the brain-mask cascade.

    probs_mask = mask_model(x)                                    2-class ResNeSt_brainMask (:221-223)
    x[round(probs_mask)[..., 0] == 1] = 0   (all ten channels)    (:224-227)
    probs = bleed_model(x)                                        3-class ResNeSt_T0 (:228-236)
    prob_map = 1 - p0 - 0.5*p1 + p2,  bleed_prob = p2             (:239, :249-252)

``Cascade`` runs it on the device for a batch: one input cast serves both models, the gate and the maps are one launch each
(csrc/cascade.hip), nothing returns to the host in between, and ``capture_predict_graph`` (``step.PredictDriver``) records the whole
cascade as ONE HIP graph.  ``Polar_Model`` is the batched form of the reference's ``Polar_Model(sAll=True)``, which starts one OS process
per image and reloads both models in each.  The plotting (``Display``) stays out: this module draws nothing, writes no file, and reads
no file when imported.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .ops import roundup
from .step import PredictDriver
from .VisionTransformer import VisionTransformer


class CascadeOutput(NamedTuple):
    probs: torch.Tensor                   # the bleed model's fp32 [B,H,W,3]
    mask: Optional[torch.Tensor]          # uint8 [B,H,W]: 1 where the input was zeroed; None without a mask model
    prob_map: torch.Tensor                # fp32 [B,H,W]: ((1 - p0) - 0.5*p1) + p2 (:249-252)
    bleed_prob: torch.Tensor              # fp32 [B,H,W]: p2 (:239)


class Cascade(PredictDriver):
    """``Cascade(bleed_model, mask_model=None)``: the bleed model (3 classes) behind an optional brain-mask model (2 classes).
    ``mask_model=None`` is the reference's ``use_brainMask=False``: the bleed model and the maps.  Both models are Arch B segmenters
    (``VisionTransformer``, the ``TBI_TransUNet`` variant included) on one device with one input geometry.  ``predict(x)`` takes
    x [B,H,W,C] (numpy or tensor, fp32 / fp64) and returns a ``CascadeOutput``; after ``capture_predict_graph`` an input of the captured
    layout replays one graph and the result holds that graph's static buffers (valid until the next call)."""

    def __init__(self, bleed_model, mask_model=None):
        models = [bleed_model] + ([mask_model] if mask_model is not None else [])
        for m in models:
            if not isinstance(m, VisionTransformer):
                raise ValueError(f"Cascade takes VisionTransformer models (TBI_TransUNet included), got {type(m).__name__}")
        if bleed_model.num_classes != 3:
            raise ValueError(f"the bleed model must have 3 classes, has {bleed_model.num_classes}")
        if mask_model is not None:
            if mask_model.num_classes != 2:
                raise ValueError(f"the brain-mask model must have 2 classes, has {mask_model.num_classes}")
            if mask_model.device != bleed_model.device:
                raise ValueError(f"the models are on {mask_model.device} and {bleed_model.device}")
            if tuple(mask_model.img_size) != tuple(bleed_model.img_size):
                raise ValueError(f"image sizes differ: mask {tuple(mask_model.img_size)}, bleed {tuple(bleed_model.img_size)}")
            if mask_model.input_shape[-1] != bleed_model.input_shape[-1]:
                raise ValueError(f"input channels differ: mask {mask_model.input_shape[-1]}, bleed {bleed_model.input_shape[-1]}")
        self.bleed_model, self.mask_model = bleed_model, mask_model
        self.device = bleed_model.device
        self.img_size = tuple(bleed_model.img_size)
        self.in_channels = bleed_model.input_shape[-1]

    @classmethod
    def from_checkpoints(cls, bleed_path, mask_path=None, *, img_size=(256, 80), in_channels=10, batch_size=16, use_vit=False,
                         transunet=False):
        """Build the models and load the files ``VisionTransformer.save`` / ``visionModel.save`` wrote (MainNumpy.py:177).
        ``transunet=True`` builds the ``TBI_TransUNet`` variant (whose ViT bottleneck is always on)."""
        def build(path, classes):
            if transunet:
                from .TBI_TransUNet import VisionTransformer as TransUNet
                m = TransUNet(img_size=img_size, num_classes=classes, batch_size=batch_size, in_channels=in_channels, seed=None)
            else:
                m = VisionTransformer(batch_size, img_size, classes, in_channels=in_channels, use_vit=use_vit, seed=None)
            m.load(path)
            return m
        return cls(build(bleed_path, 3), build(mask_path, 2) if mask_path is not None else None)

    # ------------------------------------------------------------------ PredictDriver hooks
    def _prep_x(self, x):
        x = self.bleed_model._prep_x(x)
        H, W = self.img_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (H, W, self.in_channels) or x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"expected fp32 / fp64 input [B,{H},{W},{self.in_channels}], got {x.dtype} {tuple(x.shape)}")
        return x

    def _predict_state(self):
        return self.bleed_model._predict_state() + (self.mask_model._predict_state() if self.mask_model is not None else [])

    def _predict_body(self, x):
        """cast -> mask model -> gate (in place) -> bleed model -> maps, all on the current stream, no host synchronisation."""
        xb = ops.cast_input(x, roundup(self.in_channels, 8))          # once: 0.0 is exact in bf16, so gating after the cast is exact
        mask = None
        if self.mask_model is not None:
            pm = self.mask_model._predict_body(xb)
            B, H, W = pm.shape[:3]
            mask = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
            ops.cascade_gate(pm, xb, out=xb, mask=mask)                  # the mask model has read xb: it may be overwritten
        probs = self.bleed_model._predict_body(xb)
        prob_map, bleed_prob = ops.cascade_maps(probs)
        return CascadeOutput(probs, mask, prob_map, bleed_prob)


# ---------------------------------------------------------------------------------------------------------- the test-data driver
class PolarResult(NamedTuple):
    prob_map: np.ndarray                  # fp32 [N,H,W]  (the reference's probO)
    bleed_prob: np.ndarray                # fp32 [N,H,W]  (probOut)
    mask: Optional[np.ndarray]            # uint8 [N,H,W] (None without a mask model)
    label: np.ndarray                     # [N,H,W]       (testY)
    bmode: np.ndarray                     # [N,H,W]       (bMode * -1, :247)
    names: Optional[np.ndarray]


def preProcess1(data, img_size=(256, 80)):
    """The reference's preProcess1 (:76-84) for every image at once: ``data`` [N, d1, d2, d3, 12] with d1*d2*d3 == H*W (channel 0 the
    label, 1..10 the input, 11 the B-mode image) -> (x fp32 [N,H,W,10], label [N,H,W], bmode [N,H,W] negated as at :247).  New arrays:
    ``data`` is not modified (the reference zeroes its testX in place)."""
    data = np.asarray(data)
    H, W = img_size
    if data.ndim != 5 or data.shape[-1] != 12 or int(np.prod(data.shape[1:4])) != H * W:
        raise ValueError(f"expected data [N, d1, d2, d3, 12] with d1*d2*d3 == {H}*{W}, got {data.shape}")
    N = data.shape[0]
    flat = data.reshape(N, H, W, 12)
    x = np.array(flat[..., 1:11], dtype=np.float32)        # Keras casts the float64 input to float32 before the model (:221, :235)
    label = np.array(flat[..., 0])
    bmode = np.array(flat[..., 11]) * -1
    return x, label, bmode


def batches(x, batch_size):
    """Split x [N,...] into batches of exactly ``batch_size`` images: -> [(first index, valid images, batch)], the short last batch
    padded with zero images (a captured graph has one batch shape)."""
    N = x.shape[0]
    out = []
    for lo in range(0, N, batch_size):
        n = min(batch_size, N - lo)
        xb = x[lo:lo + n]
        if n < batch_size:
            xb = np.concatenate([xb, np.zeros((batch_size - n,) + x.shape[1:], dtype=x.dtype)])
        out.append((lo, n, np.ascontiguousarray(xb)))
    return out


def Polar_Model(data, cascade: Cascade, names=None, batch_size=16):
    """The batched ``Polar_Model(sAll=True)`` (:163-207 / :210-255 without the plots): every image of ``data`` (``preProcess1``'s layout)
    through ``cascade``, ``batch_size`` images per replay of one captured HIP graph, the last batch padded with zero images whose rows
    are dropped.  -> ``PolarResult`` of NumPy arrays."""
    x, label, bmode = preProcess1(data, cascade.img_size)
    H, W = cascade.img_size
    shape = (batch_size, H, W, x.shape[-1])
    px = getattr(cascade, "_px", None)
    if cascade._pgraph is None or px is None or tuple(px.shape) != shape or px.dtype != torch.float32:
        cascade.capture_predict_graph(torch.zeros(shape, dtype=torch.float32, device=cascade.device))
    buf = cascade.predict_inputs()
    N = x.shape[0]
    prob_map = np.empty((N, H, W), np.float32)
    bleed_prob = np.empty((N, H, W), np.float32)
    mask = np.empty((N, H, W), np.uint8) if cascade.mask_model is not None else None
    for lo, n, xb in batches(x, batch_size):
        buf.copy_(torch.from_numpy(xb))
        out = cascade.predict(buf)
        prob_map[lo:lo + n] = out.prob_map[:n].cpu().numpy()
        bleed_prob[lo:lo + n] = out.bleed_prob[:n].cpu().numpy()
        if mask is not None:
            mask[lo:lo + n] = out.mask[:n].cpu().numpy()
    return PolarResult(prob_map, bleed_prob, mask, label, bmode, None if names is None else np.asarray(names))
