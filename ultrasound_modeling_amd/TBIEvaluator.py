"""The model computation of the reference's inference driver ``TBIEvaluator.py`` (``Polar_Model`` / ``PolarProcess``, duplicated in
``DisplayInference.py``) with ``use_brainMask=True``: the brain-mask cascade.

    probs_mask = mask_model(x)                                    2-class ResNeSt_brainMask (:221-223)
    x[round(probs_mask)[..., 0] == 1] = 0   (all ten channels)    (:224-227)
    probs = bleed_model(x)                                        3-class ResNeSt_T0 (:228-236)
    prob_map = 1 - p0 - 0.5*p1 + p2,  bleed_prob = p2             (:239, :249-252)

``Cascade`` runs it on the device for a batch: one input cast serves both models, the gate and the maps are one launch each
(csrc/cascade.hip), nothing returns to the host in between, and ``capture_predict_graph`` (``step.PredictDriver``) records the whole
cascade as ONE HIP graph.  ``Polar_Model`` is the batched form of the reference's ``Polar_Model(sAll=True)``, which starts one OS process
per image and reloads both models in each.

The figures (``Display``, :254-372 with the ``dispDict`` state the reference runs in): a 2x2 figure per image of four ``pcolormesh``
panels on the scan geometry of ``axis/xAxis.npy`` / ``axis/yAxis.npy`` (cast with ``astype(int)``, :19-24) - Prediction (``prob_map``,
magma, 0..2), the label (magma, 0..2), Probability Bleed (``bleed_prob``, magma, 0..1) and bMode (``binary``, from
``np.histogram(bMode, bins=25)`` edge 2 to edge -2).  ``ConeGeometry`` scan-converts the quads once (csrc/cone.hip: the largest
row-major quad whose nonzero winding number at the pixel centre is not 0, the values ``C[:-1, :-1]`` that matplotlib < 3.5 drew,
y down); ``render_figures`` colour-maps all four panels of a batch in one launch after one range launch; ``Display`` writes the PNGs
(a stdlib writer, compressed in a thread pool).  ``python -m ultrasound_modeling_amd.TBIEvaluator`` is the reference's module-level run.
Deliberate deviations from the reference's pictures:
  - no titles, axes, ticks or fonts; the panels sit on white, ``gap`` pixels apart;
  - the panel size is set by ``px_per_unit`` (pixels per axis unit), not by matplotlib's figure layout;
  - a pixel shows the quad that covers its centre, where Agg's non-antialiased fill decides by its own coverage rule (the two agree
    within one pixel: tests/test_cpu_cone.py), and the colours are matplotlib's ``bytes=True`` tables, which truncate where Agg rounds
    (a channel can be one lower);
  - a bMode image that holds a NaN or an infinity, or spans a range too small for 25 bins, raises ``ValueError``, as
    ``np.histogram`` does; NaN / infinite values of the other panels are left white (pcolormesh masks them);
  - files are overwritten, the folder is created with its parents, and ``stamp=False`` drops the ``%f`` suffix.
Importing this module draws nothing, writes no file and reads no file; matplotlib is imported only for its colormap tables.
"""
from __future__ import annotations

import argparse
import binascii
import datetime
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .ensemble import Ensemble
from .ops import roundup
from .step import PredictDriver
from .VisionTransformer import VisionTransformer


class CascadeOutput(NamedTuple):
    probs: torch.Tensor                   # the bleed model's fp32 [B,H,W,3]
    mask: Optional[torch.Tensor]          # uint8 [B,H,W]: 1 where the input was zeroed; None without a mask model
    prob_map: torch.Tensor                # fp32 [B,H,W]: ((1 - p0) - 0.5*p1) + p2 (:249-252)
    bleed_prob: torch.Tensor              # fp32 [B,H,W]: p2 (:239)


class EnsembleCascadeOutput(NamedTuple):
    probs: torch.Tensor                   # the ensemble's mean fp32 [B,H,W,3]
    mask: Optional[torch.Tensor]          # as CascadeOutput
    prob_map: torch.Tensor                # as CascadeOutput, of the mean probabilities
    bleed_prob: torch.Tensor              # as CascadeOutput, of the mean probabilities
    entropy: torch.Tensor                 # fp32 [B,H,W]: the predictive entropy of the mean (ensemble.EnsembleOutput)
    mutual_info: torch.Tensor             # fp32 [B,H,W]: what the members disagree about
    image_scores: torch.Tensor            # fp32 [B,4]: ensemble.EnsembleOutput.image_scores


class Cascade(PredictDriver):
    """``Cascade(bleed_model, mask_model=None)``: the bleed model (3 classes) behind an optional brain-mask model (2 classes).
    ``mask_model=None`` is the reference's ``use_brainMask=False``: the bleed model and the maps.  Both models are Arch B segmenters
    (``VisionTransformer``, the ``TBI_TransUNet`` variant included) on one device with one input geometry.  ``predict(x)`` takes
    x [B,H,W,C] (numpy or tensor, fp32 / fp64) and returns a ``CascadeOutput``; after ``capture_predict_graph`` an input of the captured
    layout replays one graph and the result holds that graph's static buffers (valid until the next call).
    ``bleed_model`` may be an ``ensemble.Ensemble`` of Arch B models: the mask model still runs once on the un-mirrored input and gates once, the
    gated input goes through every member, the maps come from the mean probabilities, and ``predict`` returns an ``EnsembleCascadeOutput``.
    ``temperature=T`` (``metrics.fit_temperature``'s, for one) calibrates the bleed model's probabilities in place before the maps:
    softmax(log(probs + 1e-7) / T), one more launch (``ops.apply_temperature``).  ``probs``, ``prob_map`` and ``bleed_prob`` are then all
    calibrated; one scalar cannot change the arg-max.  For an ``Ensemble`` it is the temperature of the MEAN probabilities, not one per member,
    and ``entropy`` / ``mutual_info`` / ``image_scores`` stay those of the members' un-scaled outputs.  1/T lives in a device float the kernel
    reads, so ``set_temperature`` reaches a captured predict graph without a recapture.  ``temperature=None``: no launch is added."""

    def __init__(self, bleed_model, mask_model=None, temperature=None):
        self.ensemble = isinstance(bleed_model, Ensemble)
        models = (list(bleed_model.models) if self.ensemble else [bleed_model]) + ([mask_model] if mask_model is not None else [])
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
        self._beta = None                   # fp32 [1] on the device: 1 / temperature; None until a temperature is set (no launch is added)
        if temperature is not None:
            self.set_temperature(temperature)

    @property
    def temperature(self):
        """The temperature the next ``predict`` applies, read from the device (synchronises); None when none was ever set."""
        return None if self._beta is None else 1.0 / float(self._beta.item())

    def set_temperature(self, T):
        """From the next ``predict`` on, eager or replayed: the kernel reads the device float, so a captured graph needs no recapture - unless
        it was captured before the FIRST temperature was set (it holds no temperature launch), which drops the capture."""
        beta = _beta_of(T)
        if self._beta is None:
            self._beta = torch.empty(1, dtype=torch.float32, device=self.device)
            self._pgraph = None             # a graph captured without the launch cannot follow the value
        self._beta.fill_(beta)

    @classmethod
    def from_checkpoints(cls, bleed_path, mask_path=None, *, img_size=(256, 80), in_channels=10, batch_size=16, use_vit=False,
                         transunet=False, bleed_extra=(), flip=False, temperature=None):
        """Build the models and load the files ``VisionTransformer.save`` / ``visionModel.save`` wrote (MainNumpy.py:177).
        ``transunet=True`` builds the ``TBI_TransUNet`` variant (whose ViT bottleneck is always on).  ``bleed_extra`` (more bleed checkpoints)
        or ``flip`` (left-right test-time augmentation) make the bleed model an ``Ensemble``.  ``temperature``: ``Cascade``'s."""
        def build(path, classes):
            if transunet:
                from .TBI_TransUNet import VisionTransformer as TransUNet
                m = TransUNet(img_size=img_size, num_classes=classes, batch_size=batch_size, in_channels=in_channels, seed=None)
            else:
                m = VisionTransformer(batch_size, img_size, classes, in_channels=in_channels, use_vit=use_vit, seed=None)
            m.load(path)
            return m
        bleed = build(bleed_path, 3)
        if bleed_extra or flip:
            bleed = Ensemble([bleed] + [build(p, 3) for p in bleed_extra], flip=flip)
        return cls(bleed, build(mask_path, 2) if mask_path is not None else None, temperature=temperature)

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
        if self.ensemble:
            e = self.bleed_model._predict_body(xb)
            if self._beta is not None:
                ops.apply_temperature(e.probs, self._beta, out=e.probs)     # of the mean; entropy / mutual_info / image_scores are the members'
            prob_map, bleed_prob = ops.cascade_maps(e.probs)
            return EnsembleCascadeOutput(e.probs, mask, prob_map, bleed_prob, e.entropy, e.mutual_info, e.image_scores)
        probs = self.bleed_model._predict_body(xb)
        if self._beta is not None:
            ops.apply_temperature(probs, self._beta, out=probs)
        prob_map, bleed_prob = ops.cascade_maps(probs)
        return CascadeOutput(probs, mask, prob_map, bleed_prob)


def _beta_of(T):
    """A temperature -> beta = 1/T as the kernel takes it: finite, with 1/16 <= T (beta <= 16)."""
    T = float(T)
    if not (T == T and 1.0 / 16.0 <= T < float("inf")):
        raise ValueError(f"the temperature must be a finite number >= 1/16, got {T!r}")
    return 1.0 / T


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
    return _polar_run(data, cascade, names, batch_size, uncertainty=False)[0]


class PolarUncertainty(NamedTuple):
    result: "PolarResult"
    entropy: np.ndarray                   # fp32 [N,H,W]
    mutual_info: np.ndarray               # fp32 [N,H,W]
    image_scores: np.ndarray              # fp32 [N,4] (ensemble.EnsembleOutput.image_scores)


UNCERTAINTY_COLUMNS = ("mean_entropy", "mean_mutual_info", "max_mutual_info", "mean_entropy_bleed")


def Polar_Uncertainty(data, cascade: Cascade, names=None, batch_size=16):
    """``Polar_Model`` for a cascade whose bleed model is an ``Ensemble``: -> ``PolarUncertainty`` = the same ``PolarResult`` (of the mean
    probabilities) with the NumPy ``entropy``, ``mutual_info`` [N,H,W] and ``image_scores`` [N,4]."""
    if not getattr(cascade, "ensemble", False):
        raise ValueError("Polar_Uncertainty needs a Cascade whose bleed model is an ensemble.Ensemble")
    result, extra, _ = _polar_run(data, cascade, names, batch_size, uncertainty=True)
    return PolarUncertainty(result, *extra)


def write_uncertainty_csv(path, names, image_scores):
    """One row per image: name and the four image scores (``UNCERTAINTY_COLUMNS``).  -> the number of rows."""
    import csv
    image_scores = np.asarray(image_scores)
    if image_scores.ndim != 2 or image_scores.shape[1] != 4:
        raise ValueError(f"image_scores must be [N,4], got {image_scores.shape}")
    names = [str(i) for i in range(len(image_scores))] if names is None else [str(n) for n in names]
    if len(names) != len(image_scores):
        raise ValueError(f"{len(names)} names for {len(image_scores)} images")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name"] + list(UNCERTAINTY_COLUMNS))
        for n, row in zip(names, image_scores):
            w.writerow([n] + [repr(float(v)) for v in row])
    return len(names)


def _probs_and_one_hot(result_probs, labels):
    """-> (probabilities fp32 [N,H,W,C], one-hot labels fp32 [N,H,W,C]), both contiguous NumPy arrays: ``calibration_scores``' label rule."""
    probs = np.ascontiguousarray(result_probs, dtype=np.float32)
    if probs.ndim != 4:
        raise ValueError(f"probabilities must be [N,H,W,C], got {probs.shape}")
    labels = np.asarray(labels)
    C = probs.shape[-1]
    if labels.shape == probs.shape[:3]:
        with np.errstate(invalid="ignore"):
            idx = np.clip(np.ceil(np.nan_to_num(labels.astype(np.float64)) - 0.5), 0, C - 1).astype(np.int64)
        labels = np.eye(C, dtype=np.float32)[idx]
    if labels.shape != probs.shape:
        raise ValueError(f"labels {labels.shape} match neither {probs.shape} nor {probs.shape[:3]}")
    return probs, np.ascontiguousarray(labels, dtype=np.float32)


def calibration_scores(result_probs, labels, bins=15, cls=-1, device=None, batch_size=64):
    """Reliability table and scores (``metrics.calibration_from_counts``' dict: per-bin ``n`` / ``accuracy`` / ``confidence``, ``ece``, ``mce``,
    ``brier``, ``n_invalid``) of probabilities [N,H,W,C] against labels - one-hot [N,H,W,C], or a label plane [N,H,W] as ``PolarResult.label`` (class k where
    k - 0.5 < label <= k + 0.5, clipped to the classes: ``surface_scores``' ``label > 1.5`` for the bleed class).  Counted on the device (``usseg_calibration_bins``), one read-back."""
    from .metrics import CalibrationBins
    probs, labels = _probs_and_one_hot(result_probs, labels)
    C = probs.shape[-1]
    dev = torch.device(device if device is not None else "cuda")
    cal = CalibrationBins(bins, cls, device=dev)
    if not -1 <= int(cls) < C:
        raise ValueError(f"cls must be -1 or a class below {C}, got {cls}")
    for lo in range(0, probs.shape[0], batch_size):
        cal.update(torch.from_numpy(probs[lo:lo + batch_size]).to(dev), torch.from_numpy(labels[lo:lo + batch_size]).to(dev))
    return cal.result()


def write_calibration_csv(path, scores):
    """The reliability table - one row per bin: bin, lower edge, upper edge, n, accuracy, confidence - and a final row ``total`` with the
    number of valid pixels, ECE, MCE, Brier and the invalid count.  -> the number of bin rows."""
    import csv
    bins = len(scores["n"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["bin", "lo", "hi", "n", "accuracy", "confidence", "ece", "mce", "brier", "n_invalid"])
        for b in range(bins):
            w.writerow([b, repr(b / bins), repr((b + 1) / bins), int(scores["n"][b]), repr(float(scores["accuracy"][b])),
                        repr(float(scores["confidence"][b]))] + [""] * 4)
        w.writerow(["total", "", "", int(np.sum(scores["n"])), "", "", repr(float(scores["ece"])), repr(float(scores["mce"])),
                    repr(float(scores["brier"])), int(scores["n_invalid"])])
    return bins


SWEEP_COLUMNS = ("k", "threshold", "tp", "fp", "fn", "tn", "tpr", "fpr", "precision", "dice")


def sweep_scores(result_probs, labels, bins=1024, cls=-1, device=None, batch_size=64):
    """The operating points of class ``cls`` (default: the last, the bleed class) - ``metrics.sweep_from_counts``' dict: ROC and PR points, Dice
    against the threshold, ``auc``, ``average_precision``, ``best_dice``, ``best_youden`` - of probabilities [N,H,W,C] against one-hot labels or
    a label plane, as ``calibration_scores`` takes them.  Counted on the device (``usseg_score_sweep``), one read-back.  A returned threshold
    can be passed as it is to every ``threshold=`` argument here: "bin >= k" is ``bleed_prob > threshold[k]``."""
    from .metrics import SweepCounts
    probs, labels = _probs_and_one_hot(result_probs, labels)
    C = probs.shape[-1]
    if not -C <= int(cls) < C:
        raise ValueError(f"cls must be a class below {C} (or negative, from the last), got {cls}")
    dev = torch.device(device if device is not None else "cuda")
    sw = SweepCounts(bins, cls, device=dev)
    for lo in range(0, probs.shape[0], batch_size):
        sw.update(torch.from_numpy(probs[lo:lo + batch_size]).to(dev), torch.from_numpy(labels[lo:lo + batch_size]).to(dev))
    return sw.result()


def write_roc_csv(path, scores):
    """One row per operating point (``SWEEP_COLUMNS``) and a final row ``total``: the valid pixels, AUC, average precision, the best-Dice point
    (k, threshold, Dice), the Youden point (k, threshold, J) and the invalid count.  -> the number of operating points."""
    import csv
    n = len(scores["threshold"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(SWEEP_COLUMNS) + ["n", "auc", "average_precision", "best_dice_k", "best_dice_threshold", "best_dice", "youden_k", "youden_threshold",
                                          "youden", "n_invalid"])
        for k in range(n):
            w.writerow([k, repr(float(scores["threshold"][k]))] + [int(scores[c][k]) for c in ("tp", "fp", "fn", "tn")] +
                       [repr(float(scores[c][k])) for c in ("tpr", "fpr", "precision", "dice")] + [""] * 10)
        bd, by = scores["best_dice"], scores["best_youden"]
        total = int(scores["tp"][0]) + int(scores["fp"][0])
        w.writerow(["total"] + [""] * 9 + [total, repr(float(scores["auc"])), repr(float(scores["average_precision"])), int(bd[0]), repr(float(bd[1])),
                                           repr(float(bd[2])), int(by[0]), repr(float(by[1])), repr(float(by[2])), int(scores["n_invalid"])])
    return n


def fit_cascade_temperature(probs, labels, *, lo=1 / 8, hi=8.0, candidates=16, rounds=4, device=None, batch_size=64):
    """``metrics.fit_temperature`` of un-scaled probabilities [N,H,W,C] (a run without a temperature, ``keep_probs``) against one-hot labels or
    a label plane, as ``calibration_scores`` takes them: -> its dict; ``Cascade.set_temperature(d["temperature"])`` applies it."""
    from .metrics import fit_temperature
    probs, labels = _probs_and_one_hot(probs, labels)
    dev = torch.device(device if device is not None else "cuda")
    parts = [(torch.from_numpy(probs[i:i + batch_size]).to(dev), torch.from_numpy(labels[i:i + batch_size]).to(dev))
             for i in range(0, probs.shape[0], batch_size)]
    return fit_temperature(parts, lo=lo, hi=hi, candidates=candidates, rounds=rounds, device=dev)


def _polar_run(data, cascade, names, batch_size, uncertainty, keep_probs=False):
    """The loop of ``Polar_Model`` -> (``PolarResult``, (entropy, mutual_info, image_scores) with ``uncertainty`` else None, the probabilities
    [N,H,W,3] with ``keep_probs`` else None)."""
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
    extra = None
    if uncertainty:
        extra = (np.empty((N, H, W), np.float32), np.empty((N, H, W), np.float32), np.empty((N, 4), np.float32))
    probs = np.empty((N, H, W, 3), np.float32) if keep_probs else None
    for lo, n, xb in batches(x, batch_size):
        buf.copy_(torch.from_numpy(xb))
        out = cascade.predict(buf)
        prob_map[lo:lo + n] = out.prob_map[:n].cpu().numpy()
        bleed_prob[lo:lo + n] = out.bleed_prob[:n].cpu().numpy()
        if mask is not None:
            mask[lo:lo + n] = out.mask[:n].cpu().numpy()
        if extra is not None:
            for dst, src in zip(extra, (out.entropy, out.mutual_info, out.image_scores)):
                dst[lo:lo + n] = src[:n].cpu().numpy()
        if probs is not None:
            probs[lo:lo + n] = out.probs[:n].cpu().numpy()
    result = PolarResult(prob_map, bleed_prob, mask, label, bmode, None if names is None else np.asarray(names))
    return result, extra, probs


# ---------------------------------------------------------------------------------------------------------- surface scores
def surface_scores(result: PolarResult, threshold=0.5, device=None, *, pred_mask=None, percentiles=None, tolerances=None):
    """Hausdorff and average symmetric surface distance of the bleed class, per image: the prediction ``result.bleed_prob > threshold``
    against the label's class 2 (``label > 1.5``: ``label2vec``'s class-2 plane under the 0.5 rule).  -> ``metrics.surface_distances``' dict
    (``hd`` / ``assd`` NaN for an image without a predicted or without a labelled bleed, ``n_a`` / ``n_b`` the two surface pixel counts).
    ``pred_mask`` [N,H,W] (``clean_result``'s, for one) is scored in place of ``bleed_prob > threshold``.  ``percentiles`` (95 for HD95) and
    ``tolerances`` (pixels) add ``hd_pct``, ``hd_pct_directed`` and ``nsd`` (``metrics.surface_scores_from_stats``)."""
    from .metrics import surface_distances
    pred = np.asarray(result.bleed_prob) > threshold if pred_mask is None else np.asarray(pred_mask) != 0
    if percentiles is None and tolerances is None:
        return surface_distances(pred, np.asarray(result.label) > 1.5, device=device)
    return surface_distances(pred, np.asarray(result.label) > 1.5, device=device, percentiles=percentiles, tolerances=tolerances)


def _column_number(v):
    """95.0 -> "95", 99.9 -> "99.9": the number as it reads in a column name."""
    v = float(v)
    return str(int(v)) if v == int(v) else repr(v)


def write_surface_csv(path, result: PolarResult, threshold=0.5, device=None, *, pred_mask=None, percentiles=None, tolerances=None):
    """One row per image: name, hd, assd, surface pixels of the prediction, surface pixels of the label; with ``percentiles`` / ``tolerances``
    also hd<q> (pooled, medpy's), hd<q>_directed (MONAI's) per percentile and nsd<tau> per tolerance.  -> the number of rows."""
    import csv
    extra = percentiles is not None or tolerances is not None
    if extra:
        s = surface_scores(result, threshold, device=device, pred_mask=pred_mask, percentiles=percentiles, tolerances=tolerances)
    else:
        s = surface_scores(result, threshold, device=device, pred_mask=pred_mask)
    names = _names(result)
    head = ["name", "hd", "assd", "n_pred", "n_label"]
    if extra:
        for q in s["percentiles"]:
            head += [f"hd{_column_number(q)}", f"hd{_column_number(q)}_directed"]
        head += [f"nsd{_column_number(t)}" for t in s["tolerances"]]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(head)
        for i, n in enumerate(names):
            row = [n, repr(float(s["hd"][i])), repr(float(s["assd"][i])), int(s["n_a"][i]), int(s["n_b"][i])]
            if extra:
                for p in range(len(s["percentiles"])):
                    row += [repr(float(s["hd_pct"][i][p])), repr(float(s["hd_pct_directed"][i][p]))]
                row += [repr(float(s["nsd"][i][t])) for t in range(len(s["tolerances"]))]
            w.writerow(row)
    return len(names)


# ---------------------------------------------------------------------------------------------------------- lesions
def clean_result(result: PolarResult, threshold=0.5, *, min_area, min_peak=0.0, connectivity=8, device=None):
    """The cleaned bleed mask, uint8 [N,H,W] (NumPy): ``bleed_prob > threshold`` without the connected components of fewer than ``min_area``
    pixels or whose largest ``bleed_prob`` is below ``min_peak`` (usseg.h ``usseg_clean_mask``, on the device)."""
    dev = torch.device(device if device is not None else "cuda")
    prob = torch.from_numpy(np.ascontiguousarray(result.bleed_prob, dtype=np.float32)).to(dev)
    if prob.dim() != 3:
        raise ValueError(f"bleed_prob must be [N,H,W], got {tuple(prob.shape)}")
    mask = (prob > threshold).to(torch.uint8)
    return ops.clean_mask(mask, prob, connectivity=connectivity, min_area=min_area, min_peak=min_peak, out=mask).cpu().numpy()


def lesion_scores(result: PolarResult, threshold=0.5, *, min_area=1, min_peak=0.0, connectivity=8, device=None):
    """Lesion-wise detection scores of the bleed class (``metrics.lesion_scores``): the cleaned prediction (``clean_result``) against the
    labelled lesions, the components of ``label > 1.5``."""
    from .metrics import lesion_scores as scores
    pred = clean_result(result, threshold, min_area=min_area, min_peak=min_peak, connectivity=connectivity, device=device)
    return scores(pred, np.asarray(result.label) > 1.5, connectivity=connectivity, device=device)


LESION_COLUMNS = ("n_true", "n_pred", "detected", "missed", "false_pos", "largest_true", "largest_pred")


def write_lesion_csv(path, result: PolarResult, threshold=0.5, *, min_area=1, min_peak=0.0, connectivity=8, device=None):
    """One row per image - name and ``LESION_COLUMNS`` - and a final row ``total`` with the column sums (the two ``largest`` columns: the
    maxima) followed by sensitivity, precision, f1 and false positives per image over the stack.  -> the number of image rows."""
    import csv
    s = lesion_scores(result, threshold, min_area=min_area, min_peak=min_peak, connectivity=connectivity, device=device)
    names = _names(result)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name"] + list(LESION_COLUMNS) + ["sensitivity", "precision", "f1", "fp_per_image"])
        for i, n in enumerate(names):
            w.writerow([n] + [int(s[c][i]) for c in LESION_COLUMNS] + [""] * 4)
        tot = [int(s[c].max(initial=0)) if c.startswith("largest") else int(s[c].sum()) for c in LESION_COLUMNS]
        w.writerow(["total"] + tot + [repr(float(s[k])) for k in ("sensitivity", "precision", "f1", "fp_per_image")])
    return len(names)


# ---------------------------------------------------------------------------------------------------------- per-image / per-patient scores
def image_scores(result: PolarResult, geometry=None, threshold=0.5, pred_mask=None, device=None):
    """The bleed class's overlap table per image (``metrics.image_scores``): the prediction ``result.bleed_prob > threshold`` - or
    ``pred_mask`` [N,H,W], as ``surface_scores`` takes it - against the label's class 2 (``label > 1.5``).  ``geometry``: a
    ``metrics.ScanGeometry`` (the axes UNCAST) adds the areas in axis units^2."""
    from .metrics import image_scores as scores
    pred = np.asarray(result.bleed_prob) > threshold if pred_mask is None else np.asarray(pred_mask) != 0
    return scores(pred, np.asarray(result.label) > 1.5, geometry, device=device)


SCORE_COLUMNS = ("tp", "fp", "fn", "tn", "dice", "iou", "sensitivity", "precision")
AREA_COLUMNS = ("area_true", "area_pred", "area_tp", "area_dice", "area_error")


def _cell(v):
    """An integer as it is, a float by ``repr`` (round-trips), nothing for None."""
    if v is None:
        return ""
    return int(v) if isinstance(v, (int, np.integer)) else repr(float(v))


def _summary_rows(summary, columns, lead):
    """The rows under a score table: ``pooled`` (the scores of the summed counts), ``mean`` / ``median`` over the defined entries and
    ``defined`` (how many those are) in the ratio columns; with areas ``loa_lower`` / ``loa_upper`` (Bland-Altman: bias -+ 1.96 sd; the bias
    is the ``mean`` row's ``area_error``) in the ``area_error`` column; with a bootstrap ``ci_pooled_lower`` / ``ci_pooled_upper`` (pooled Dice
    under ``dice``, pooled area Dice under ``area_dice``, TOTAL area error under ``area_error``) and ``ci_mean_lower`` / ``ci_mean_upper``
    (the mean per-image Dice under ``dice``).  ``lead``: the cells between the row's name and the first score column."""
    def row(name, values):
        return [name] + list(lead) + [_cell(values.get(c)) for c in columns]
    ba = summary.get("bland_altman")
    mean = dict(summary["mean"], **({"area_error": ba["bias"]} if ba else {}))
    rows = [row("pooled", summary["pooled"]), row("mean", mean), row("median", summary["median"]), row("defined", summary["defined"])]
    if ba:
        rows += [row("loa_lower", {"area_error": ba["lower"]}), row("loa_upper", {"area_error": ba["upper"]})]
    bs = summary.get("bootstrap")
    if bs:
        iv = bs["intervals"]
        for side, name in enumerate(("lower", "upper")):
            pooled = {"dice": iv["pooled_dice"][side]}
            if "area_dice" in iv:
                pooled.update(area_dice=iv["area_dice"][side], area_error=iv["area_error_total"][side])
            rows.append(row(f"ci_pooled_{name}", pooled))
        rows += [row(f"ci_mean_{name}", {"dice": iv["mean_dice"][side]}) for side, name in enumerate(("lower", "upper"))]
    return rows


def write_scores_csv(path, result: PolarResult, geometry=None, threshold=0.5, *, pred_mask=None, bootstrap=0, seed=0, alpha=0.05, device=None):
    """One row per image - name, ``SCORE_COLUMNS`` and with a geometry ``AREA_COLUMNS`` (an undefined ratio reads ``nan``) - then
    ``_summary_rows``.  ``bootstrap`` = R adds the percentile intervals of R replicates that resample images (``write_patient_csv``'s
    resample patients).  -> the number of image rows."""
    import csv
    from .metrics import summarize
    t = image_scores(result, geometry, threshold, pred_mask, device=device)
    names = _names(result)
    columns = SCORE_COLUMNS + (AREA_COLUMNS if geometry is not None else ())
    s = summarize(t, bootstrap=bootstrap, seed=seed, alpha=alpha, device=device)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name"] + list(columns))
        for i, n in enumerate(names):
            w.writerow([n] + [_cell(t[c][i]) for c in columns])
        w.writerows(_summary_rows(s, columns, ()))
    return len(names)


def write_patient_csv(path, result: PolarResult, geometry=None, threshold=0.5, *, pred_mask=None, pattern=r"DoD(\d+)", bootstrap=0, seed=0,
                      alpha=0.05, device=None):
    """One row per patient (``metrics.patient_of`` of each image name under ``pattern``) - patient, n_images, and the columns of
    ``write_scores_csv`` from the patient's summed counts - then ``_summary_rows`` over the PATIENTS' table (mean, median and limits of
    agreement across patients; pooled = the whole run), its bootstrap a cluster bootstrap that resamples patients.  -> the number of
    patient rows."""
    import csv
    from .metrics import grouped, patient_of, summarize
    t = image_scores(result, geometry, threshold, pred_mask, device=device)
    groups = [patient_of(n, pattern) for n in _names(result)]
    g = grouped(t, groups)
    columns = SCORE_COLUMNS + (AREA_COLUMNS if geometry is not None else ())
    s = summarize(g, bootstrap=0)
    if bootstrap:
        # the cluster bootstrap keeps the per-IMAGE Dice inside each patient's row (dice_q, dice_n), so it is drawn from the image table
        s["bootstrap"] = summarize(t, groups=groups, bootstrap=bootstrap, seed=seed, alpha=alpha, device=device)["bootstrap"]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["patient", "n_images"] + list(columns))
        for i, p in enumerate(g["groups"]):
            w.writerow([p, int(g["n_images"][i])] + [_cell(g[c][i]) for c in columns])
        w.writerows(_summary_rows(s, columns, (int(g["n_images"].sum()),)))
    return len(g["groups"])


LESION_SIZE_COLUMNS = ("pixels", "area", "diameter", "centroid_x", "centroid_y", "x_min", "x_max", "y_min", "y_max")


def write_lesion_size_csv(path, result: PolarResult, geometry, threshold=0.5, *, min_area=1, min_peak=0.0, connectivity=8, device=None):
    """One row per predicted and per labelled bleed component: name, kind (``pred`` / ``true``), id (``scipy.ndimage.label``'s numbering),
    ``LESION_SIZE_COLUMNS`` in axis units (``metrics.lesion_sizes_from_measure``) and ``matched`` = 1 when at least one of its pixels lies
    inside a component of the other kind (``ops.component_overlap``), else 0.  The prediction is the cleaned one (``clean_result``), as in
    ``write_lesion_csv``.  -> the number of component rows."""
    import csv
    from .metrics import _lesion_measure, _mask_stack, lesion_sizes_from_measure
    dev = torch.device(device if device is not None else "cuda")
    pred = clean_result(result, threshold, min_area=min_area, min_peak=min_peak, connectivity=connectivity, device=dev)
    lp, cp, mp = _lesion_measure(_mask_stack(pred, dev, "write_lesion_size_csv"), geometry, connectivity)
    lt, ct, mt = _lesion_measure(_mask_stack(np.asarray(result.label) > 1.5, dev, "write_lesion_size_csv"), geometry, connectivity)
    hit_p, hit_t = ops.component_overlap(lp, lt, mp.shape[1], mt.shape[1])
    tables = (("pred", cp, lesion_sizes_from_measure(cp, mp, geometry), hit_p.cpu().numpy()),
              ("true", ct, lesion_sizes_from_measure(ct, mt, geometry), hit_t.cpu().numpy()))
    rows = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "kind", "id"] + list(LESION_SIZE_COLUMNS) + ["matched"])
        for i, n in enumerate(_names(result)):
            for kind, count, s, hit in tables:
                for k in range(int(count[i])):
                    w.writerow([n, kind, k + 1] + [_cell(s[c][i, k]) for c in LESION_SIZE_COLUMNS] + [int(hit[i, k] > 0)])
                    rows += 1
    return rows


def _add_score_arguments(ap):
    ap.add_argument("--scores-csv", default=None, metavar="PATH",
                    help="also write the bleed class's overlap table, one row per image (tp, fp, fn, tn, Dice, IoU, sensitivity, precision and the "
                         "areas in axis units^2 from axis_dir's UNCAST axes) and summary rows")
    ap.add_argument("--patient-csv", default=None, metavar="PATH", help="the same table per patient (--patient-regex), from each patient's summed counts")
    ap.add_argument("--lesion-size-csv", default=None, metavar="PATH",
                    help="also write one row per predicted and per labelled bleed component: its area, equivalent diameter, centroid and extent in axis units")
    ap.add_argument("--patient-regex", default=r"DoD(\d+)", metavar="RE", help="what names a patient inside an image name (its first group)")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="R",
                    help="add percentile intervals from R bootstrap replicates to --scores-csv (resampling images) and --patient-csv (resampling patients)")
    ap.add_argument("--bootstrap-seed", type=int, default=0, metavar="S", help="the seed of --bootstrap")


def _check_score_arguments(ap, a):
    import re
    if not 0 <= a.bootstrap <= 1 << 20:
        ap.error("--bootstrap must lie in 0..2^20")
    if not 0 <= a.bootstrap_seed < 1 << 64:
        ap.error("--bootstrap-seed must lie in 0..2^64-1")
    if a.bootstrap and a.scores_csv is None and a.patient_csv is None:
        ap.error("--bootstrap needs --scores-csv or --patient-csv")
    try:
        re.compile(a.patient_regex)
    except re.error as e:
        ap.error(f"--patient-regex: {e}")


def _write_score_outputs(a, result, thr, device):
    """``main``'s --scores-csv / --patient-csv / --lesion-size-csv; nothing is read, imported or launched without one of them."""
    if a.scores_csv is None and a.patient_csv is None and a.lesion_size_csv is None:
        return
    from .metrics import ScanGeometry
    scan = ScanGeometry.from_dir(a.axis_dir)
    clean = dict(min_area=a.min_area if a.min_area is not None else 1, min_peak=a.min_peak, connectivity=a.connectivity)
    if a.scores_csv is not None or a.patient_csv is not None:
        cleaned = clean_result(result, **thr, **clean, device=device)
        if a.scores_csv is not None:
            rows = write_scores_csv(a.scores_csv, result, scan, pred_mask=cleaned, bootstrap=a.bootstrap, seed=a.bootstrap_seed, device=device)
            print(f"wrote {rows} image-score rows to {a.scores_csv}")
        if a.patient_csv is not None:
            rows = write_patient_csv(a.patient_csv, result, scan, pred_mask=cleaned, pattern=a.patient_regex, bootstrap=a.bootstrap, seed=a.bootstrap_seed,
                                     device=device)
            print(f"wrote {rows} patient rows to {a.patient_csv}")
    if a.lesion_size_csv is not None:
        rows = write_lesion_size_csv(a.lesion_size_csv, result, scan, **thr, **clean, device=device)
        print(f"wrote {rows} lesion-size rows to {a.lesion_size_csv}")


# ---------------------------------------------------------------------------------------------------------- the figures
PANEL_RANGES = ((0.0, 2.0), (0.0, 2.0), (0.0, 1.0))     # Prediction, label, Probability Bleed (:297, :304, :333); bMode per image
GAP = 16                                                # white pixels between the panels


def colormap_tables():
    """uint8 [2,256,3]: matplotlib's magma and binary tables (``Colormap(range(256), bytes=True)``), read at run time."""
    try:
        import matplotlib
    except ImportError as e:
        raise RuntimeError("the evaluator's figures need matplotlib for the magma / binary colormap tables; it is not installed") from e
    return np.stack([np.asarray(matplotlib.colormaps[n](range(256), bytes=True))[:, :3] for n in ("magma", "binary")]).astype(np.uint8)


class ConeGeometry:
    """The scan geometry of the figures: vertex grids ``xAxis``, ``yAxis`` [H,W] (the reference casts them with ``astype(int)``,
    :23-24; ``int_axes=False`` keeps them as they are) and ``px_per_unit`` pixels per axis unit.  Builds the panel's index image on
    ``device`` once (one ``usseg_cone_index`` launch): int32 [Hp,Wp], the quad each pixel shows or -1, with
    Hp = ceil((ymax-ymin)*px_per_unit), Wp = ceil((xmax-xmin)*px_per_unit), row 0 at ymin (the inverted y axis, :300)."""

    def __init__(self, xAxis, yAxis, px_per_unit=2, int_axes=True, device="cuda", gap=GAP):
        X, Y = np.asarray(xAxis), np.asarray(yAxis)
        if X.shape != Y.shape or X.ndim != 2 or min(X.shape) < 2:
            raise ValueError(f"xAxis {X.shape} and yAxis {Y.shape} must be one [H,W] vertex grid with H, W >= 2")
        if not (np.issubdtype(X.dtype, np.number) and np.issubdtype(Y.dtype, np.number)) or not (np.isfinite(X).all() and np.isfinite(Y).all()):
            raise ValueError("xAxis and yAxis must hold finite numbers")
        if int_axes:
            X, Y = X.astype(int), Y.astype(int)
        X, Y = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(Y, np.float64)
        ppu = float(px_per_unit)
        if not (np.isfinite(ppu) and ppu > 0):
            raise ValueError(f"px_per_unit must be a positive number, got {px_per_unit!r}")
        gap = int(gap)
        if gap < 0:
            raise ValueError(f"gap must be >= 0, got {gap}")
        self.xmin, self.ymin = float(X.min()), float(Y.min())
        Hp, Wp = int(np.ceil((Y.max() - self.ymin) * ppu)), int(np.ceil((X.max() - self.xmin) * ppu))
        if Hp < 1 or Wp < 1:
            raise ValueError(f"the grid spans no area at px_per_unit {ppu} (panel {Hp} x {Wp})")
        if Hp * Wp * 4 > ops._INT32_MAX or (2 * Hp + gap) * (2 * Wp + gap) * 3 > ops._INT32_MAX:
            raise ValueError(f"a {Hp} x {Wp} panel at px_per_unit {ppu} overflows int32 byte offsets")
        self.X, self.Y, self.px_per_unit, self.gap = X, Y, ppu, gap
        self.grid = X.shape
        self.panel = (Hp, Wp)
        self.figure_shape = (2 * Hp + gap, 2 * Wp + gap, 3)
        self.device = torch.device(device)
        self.index = ops.cone_index(torch.from_numpy(X).to(self.device), torch.from_numpy(Y).to(self.device), self.xmin, self.ymin, ppu,
                                    Hp, Wp)
        self._luts = None

    @classmethod
    def from_dir(cls, axis_dir, **kw):
        """Read ``xAxis.npy`` and ``yAxis.npy`` (``DataFilePlayGround.FetchPolarAxis``'s output) from ``axis_dir``."""
        return cls(np.load(os.path.join(axis_dir, "xAxis.npy")), np.load(os.path.join(axis_dir, "yAxis.npy")), **kw)

    def luts(self):
        if self._luts is None:
            self._luts = torch.from_numpy(colormap_tables()).to(self.device)
        return self._luts


def _check_result(result, geometry, batch_size):
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    planes = (result.prob_map, result.label, result.bleed_prob, result.bmode)
    shapes = {np.shape(p) for p in planes}
    if len(shapes) != 1 or len(next(iter(shapes))) != 3:
        raise ValueError(f"prob_map, label, bleed_prob and bmode must be one [N,H,W] shape, got {[np.shape(p) for p in planes]}")
    H, W = next(iter(shapes))[1:]
    if (H, W) != tuple(geometry.grid):
        raise ValueError(f"the maps are {H} x {W} but the geometry's vertex grid is {tuple(geometry.grid)}")


def _render_batches(result: PolarResult, geometry: ConeGeometry, batch_size):
    """-> iterator of (first index, valid images, uint8 [valid, *figure_shape] on the host): per batch one upload of the four planes,
    one ``usseg_cone_range`` and one ``usseg_cone_render`` launch; the short last batch is padded as ``batches`` pads."""
    _check_result(result, geometry, batch_size)
    dev = geometry.device
    luts = geometry.luts()
    planes = [np.asarray(result.prob_map, np.float32), np.asarray(result.label, np.float64), np.asarray(result.bleed_prob, np.float32),
              np.asarray(result.bmode, np.float64)]
    split = [batches(p, batch_size) for p in planes]
    for parts in zip(*split):
        lo, n = parts[0][0], parts[0][1]
        pm, lab, bp, bm = (torch.from_numpy(p[2]).to(dev) for p in parts)
        rng, bad = ops.cone_range(bm)
        out = ops.cone_render(geometry.index, pm, lab, bp, bm, PANEL_RANGES, rng, luts, geometry.gap)
        bad = bad[:n].cpu().numpy()
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            name = "" if result.names is None else f" ({result.names[lo + k]})"
            why = "holds NaN or infinite values" if bad[k] & 1 else "spans too small a range for 25 finite-sized bins"
            raise ValueError(f"the bMode plane of image {lo + k}{name} {why}: np.histogram cannot take its range")
        yield lo, n, out[:n].cpu().numpy()


def render_figures(result: PolarResult, geometry: ConeGeometry, batch_size=16):
    """Every image's figure: uint8 [N, 2*Hp+gap, 2*Wp+gap, 3] (NumPy), panels Prediction | label over Probability Bleed | bMode."""
    N = np.shape(result.prob_map)[0]
    figs = np.empty((N,) + geometry.figure_shape, np.uint8)
    for lo, n, f in _render_batches(result, geometry, batch_size):
        figs[lo:lo + n] = f
    return figs


def write_png(path, rgb, level=6):
    """uint8 [H,W,3] -> an 8-bit RGB PNG (filter 0 on every row, one zlib stream)."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or min(rgb.shape[:2]) < 1:
        raise ValueError(f"write_png takes uint8 [H,W,3], got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    raw = np.empty((H, 1 + 3 * W), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = rgb.reshape(H, 3 * W)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", binascii.crc32(kind + data) & 0xFFFFFFFF)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
           chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


def _names(result):
    N = np.shape(result.prob_map)[0]
    names = [str(i) for i in range(N)] if result.names is None else [str(n) for n in result.names]
    if len(names) != N:
        raise ValueError(f"{len(names)} names for {N} images")
    for n in names:
        if "/" in n or "\0" in n:
            raise ValueError(f"image name {n!r} holds a '/' (or a NUL): it would not name a file in the output folder")
    return names


def Display(result: PolarResult, geometry: ConeGeometry, savePath, stamp=True, batch_size=16, workers=16):
    """Write every image's figure to ``savePath/<%m%d-%H>/<str(name)><%f>.png`` (:346-351; ``str`` of the name as the reference
    executes it, the brackets of a row of an [N,1] paths array included; the image index when ``result.names`` is None).
    ``stamp=False`` drops the ``%f`` suffix.  Rendering runs on the device one batch ahead of the PNG compression, which a pool of at
    most 16 threads does.  -> the list of paths written, in image order."""
    names = _names(result)
    _check_result(result, geometry, batch_size)
    workers = max(1, min(16, int(workers), os.cpu_count() or 1))
    paths = [None] * len(names)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        jobs = []
        for lo, n, figs in _render_batches(result, geometry, batch_size):
            for k in range(n):
                now = datetime.datetime.now()
                folder = os.path.join(savePath, now.strftime("%m%d-%H"))
                os.makedirs(folder, exist_ok=True)
                paths[lo + k] = os.path.join(folder, names[lo + k] + (now.strftime("%f") if stamp else "") + ".png")
                jobs.append(pool.submit(write_png, paths[lo + k], figs[k]))
        for j in jobs:
            j.result()
    return paths


def main(argv=None):
    """The reference's module-level run (:375, ``Polar_Model(sAll=True)``): the test set through the cascade, then one figure per image."""
    ap = argparse.ArgumentParser(description="Test images -> the evaluator's maps and one four-panel cone figure (PNG) per image.")
    ap.add_argument("data", help="test data .npy [N, d1, d2, d3, 12] (DataFilePlayGround's output)")
    ap.add_argument("paths", help="the image names .npy (one per test image)")
    ap.add_argument("axis_dir", help="folder holding xAxis.npy and yAxis.npy")
    ap.add_argument("out", help="output folder: <out>/<%%m%%d-%%H>/<name><%%f>.png")
    ap.add_argument("--bleed", required=True, help="bleed model checkpoint (3 classes)")
    ap.add_argument("--mask", default=None, help="brain-mask model checkpoint (2 classes): the use_brainMask=True cascade")
    ap.add_argument("--batch", type=int, default=16, help="images per graph replay and per render launch")
    ap.add_argument("--px-per-unit", type=float, default=2.0, help="panel pixels per axis unit")
    ap.add_argument("--no-stamp", action="store_true", help="name files <name>.png, without the %%f suffix")
    ap.add_argument("--transunet", action="store_true", help="the checkpoints are TBI_TransUNet models")
    ap.add_argument("--use-vit", action="store_true", help="the checkpoints have the ViT bottleneck")
    ap.add_argument("--surface-csv", default=None, metavar="PATH",
                    help="also write the bleed class's Hausdorff and average symmetric surface distance, one row per image")
    ap.add_argument("--surface-percentile", type=float, action="append", default=None, metavar="Q",
                    help="add hd<Q> (pooled) and hd<Q>_directed columns to --surface-csv: the Q-th percentile of the surface distances, 95 for HD95 "
                         "(repeatable, up to 4)")
    ap.add_argument("--surface-tolerance", type=float, action="append", default=None, metavar="T",
                    help="add an nsd<T> column to --surface-csv: the surface Dice at a tolerance of T pixels (repeatable, up to 4)")
    ap.add_argument("--lesion-csv", default=None, metavar="PATH",
                    help="also write the bleed class's lesion-wise detection counts, one row per image and a totals row")
    ap.add_argument("--min-area", type=int, default=None, metavar="N",
                    help="drop predicted bleed components of fewer than N pixels before --lesion-csv / --surface-csv score them")
    ap.add_argument("--min-peak", type=float, default=0.0, metavar="P", help="drop predicted bleed components whose largest probability is below P (--lesion-csv; --surface-csv only together with --min-area)")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8), help="pixel connectivity of a component")
    ap.add_argument("--tta", default=None, choices=("flip",), help="test-time augmentation of the bleed model: flip = average with the left-right mirror")
    ap.add_argument("--bleed-extra", action="append", default=None, metavar="CKPT",
                    help="one more bleed checkpoint to ensemble with --bleed (repeatable; at most 16 members with --tta)")
    ap.add_argument("--uncertainty-csv", default=None, metavar="PATH",
                    help="write the ensemble's image scores (mean entropy, mean / max mutual information, mean entropy over the predicted bleed), "
                         "one row per image; needs --tta or --bleed-extra")
    ap.add_argument("--calibration-csv", default=None, metavar="PATH",
                    help="write the reliability table of the bleed model's (or the ensemble's mean) probabilities with ECE, MCE and the Brier score")
    ap.add_argument("--calibration-bins", type=int, default=15, metavar="N", help="confidence bins of --calibration-csv (1..64)")
    ap.add_argument("--roc-csv", default=None, metavar="PATH",
                    help="write the bleed class's threshold sweep: one row per operating point (ROC and PR points, Dice) and a total row with AUC, "
                         "average precision and the best-Dice and Youden points")
    ap.add_argument("--sweep-bins", type=int, default=1024, metavar="N", help="score bins of the sweep: a power of two in 2..4096")
    ap.add_argument("--temperature", type=float, default=None, metavar="T", help="calibrate the bleed probabilities: softmax(log(p + 1e-7) / T)")
    ap.add_argument("--fit-temperature", action="store_true",
                    help="fit the temperature on this run's data (it needs the labels), print it with the NLL and the ECE before and after, and predict again with it")
    ap.add_argument("--threshold", default=None, metavar="T|best-dice|youden",
                    help="the bleed threshold --surface-csv and --lesion-csv use (default 0.5): a number, or the sweep's best-Dice or Youden point")
    _add_score_arguments(ap)
    a = ap.parse_args(argv)
    _check_score_arguments(ap, a)
    threshold = None
    if a.threshold is not None and a.threshold not in ("best-dice", "youden"):
        try:
            threshold = float(a.threshold)
        except ValueError:
            ap.error("--threshold takes a number, best-dice or youden")
        if not threshold == threshold:
            ap.error("--threshold must not be NaN")
    if a.sweep_bins < 2 or a.sweep_bins > 4096 or a.sweep_bins & (a.sweep_bins - 1):
        ap.error("--sweep-bins must be a power of two in 2..4096")
    if a.temperature is not None and a.fit_temperature:
        ap.error("--temperature and --fit-temperature exclude each other")
    if a.temperature is not None and not (a.temperature == a.temperature and 1.0 / 16.0 <= a.temperature < float("inf")):
        ap.error("--temperature must be a finite number >= 1/16")
    sweep = a.roc_csv is not None or a.threshold in ("best-dice", "youden")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    if a.min_area is not None and a.min_area < 1:
        ap.error("--min-area must be >= 1")
    if not 0.0 <= a.min_peak <= 1.0:
        ap.error("--min-peak must lie in [0, 1]")
    if (a.surface_percentile is not None or a.surface_tolerance is not None) and a.surface_csv is None:
        ap.error("--surface-percentile / --surface-tolerance need --surface-csv")
    if len(a.surface_percentile or ()) > 4 or len(a.surface_tolerance or ()) > 4:
        ap.error("at most 4 --surface-percentile and 4 --surface-tolerance")
    if not all(0.0 <= q <= 100.0 for q in a.surface_percentile or ()):
        ap.error("--surface-percentile must lie in [0, 100]")
    if not all(0.0 <= t < float("inf") for t in a.surface_tolerance or ()):
        ap.error("--surface-tolerance must be finite and >= 0")
    ensemble = a.tta is not None or bool(a.bleed_extra)
    if a.uncertainty_csv is not None and not ensemble:
        ap.error("--uncertainty-csv needs an ensemble: --tta flip and / or --bleed-extra")
    if not 1 <= a.calibration_bins <= 64:
        ap.error("--calibration-bins must lie in 1..64")
    if (1 + len(a.bleed_extra or ())) * (2 if a.tta else 1) > 16:
        ap.error("at most 16 ensemble members (checkpoints x views)")
    data = np.load(a.data)
    names = np.load(a.paths)
    cascade = Cascade.from_checkpoints(a.bleed, a.mask, batch_size=a.batch, use_vit=a.use_vit, transunet=a.transunet,
                                       bleed_extra=tuple(a.bleed_extra or ()), flip=a.tta == "flip")
    geometry = ConeGeometry.from_dir(a.axis_dir, px_per_unit=a.px_per_unit, device=cascade.device)
    if a.temperature is not None:
        cascade.set_temperature(a.temperature)
    if a.fit_temperature:
        result, _, probs = _polar_run(data, cascade, names, a.batch, uncertainty=False, keep_probs=True)
        fit = fit_cascade_temperature(probs, result.label, device=cascade.device)
        before = calibration_scores(probs, result.label, bins=a.calibration_bins, device=cascade.device)
        cascade.set_temperature(fit["temperature"])
        _, _, probs = _polar_run(data, cascade, names, a.batch, uncertainty=False, keep_probs=True)
        after = calibration_scores(probs, result.label, bins=a.calibration_bins, device=cascade.device)
        print("fitted temperature T = {!r} (beta = {!r}): NLL {:.6f} -> {:.6f}, ECE {:.5f} -> {:.5f}".format(
            fit["temperature"], fit["beta"], fit["nll_at_1"], fit["nll"], before["ece"], after["ece"]))
    if ensemble or a.calibration_csv is not None or sweep:
        result, extra, probs = _polar_run(data, cascade, names, a.batch, uncertainty=ensemble, keep_probs=a.calibration_csv is not None or sweep)
        if a.uncertainty_csv is not None:
            rows = write_uncertainty_csv(a.uncertainty_csv, _names(result), extra[2])
            print(f"wrote {rows} uncertainty rows to {a.uncertainty_csv}")
        if a.calibration_csv is not None:
            rows = write_calibration_csv(a.calibration_csv, calibration_scores(probs, result.label, bins=a.calibration_bins, device=cascade.device))
            print(f"wrote {rows} reliability bins to {a.calibration_csv}")
        if sweep:
            from .metrics import sweep_line
            sw = sweep_scores(probs, result.label, bins=a.sweep_bins, device=cascade.device)
            print(sweep_line(sw))
            if a.roc_csv is not None:
                rows = write_roc_csv(a.roc_csv, sw)
                print(f"wrote {rows} operating points to {a.roc_csv}")
            if a.threshold in ("best-dice", "youden"):
                threshold = sw["best_dice" if a.threshold == "best-dice" else "best_youden"][1]
                print(f"--threshold {a.threshold}: {threshold!r}")
    else:
        result = Polar_Model(data, cascade, names=names, batch_size=a.batch)
    thr = {} if threshold is None else {"threshold": threshold}          # (absent: every consumer's own default, 0.5)
    if a.surface_csv is not None:
        cleaned = None
        if a.min_area is not None:
            cleaned = clean_result(result, **thr, min_area=a.min_area, min_peak=a.min_peak, connectivity=a.connectivity, device=cascade.device)
        rows = write_surface_csv(a.surface_csv, result, **thr, device=cascade.device, pred_mask=cleaned, percentiles=a.surface_percentile,
                                 tolerances=a.surface_tolerance)
        print(f"wrote {rows} surface-score rows to {a.surface_csv}")
    if a.lesion_csv is not None:
        rows = write_lesion_csv(a.lesion_csv, result, **thr, min_area=a.min_area if a.min_area is not None else 1, min_peak=a.min_peak,
                                connectivity=a.connectivity, device=cascade.device)
        print(f"wrote {rows} lesion rows to {a.lesion_csv}")
    _write_score_outputs(a, result, thr, cascade.device)
    paths = Display(result, geometry, a.out, stamp=not a.no_stamp, batch_size=a.batch)
    print(f"wrote {len(paths)} figures under {a.out}")


if __name__ == "__main__":
    main()
