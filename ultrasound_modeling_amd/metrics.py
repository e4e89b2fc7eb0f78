"""The drivers' validation metrics (MainNumpy.py:17-27,49-53,97-147; TBI_ResNest.py:9-12,413-449; TBI_TransUNet.py:749-756,
893-898,947-990; MainParallel.py:86-114,148-176) from exact device-side counters.

The reference updates five Keras metric objects per batch - Precision, Recall, MeanIoU(num_classes) and a second
Precision / Recall pair named ``c2`` - and reads them back on the host; under MirroredStrategy it also gathers every replica's
probabilities and labels.  Here one launch per batch (``ops.seg_counts`` -> ``usseg_seg_counts``) adds into a small int64
counter buffer that stays in HBM until the epoch ends; ``SegMetrics.result()`` copies it back once and ``counts_to_metrics``
turns it into the numbers the drivers print.  Replicas exchange the counters (a SUM all-reduce of 23 int64) instead of the
tensors: the sum is exact, so N replicas give the numbers of one process on the concatenated batch.

Two behaviours of the reference, reproduced on purpose:
  * ``c2`` is the last image COLUMN, not class 2: ``y[:, :, -1]`` indexes the width axis of the 4-D tensor (MainNumpy.py:104-105).
  * The counts are exact 64-bit integers; Keras keeps its counters in fp32 variables, inexact past 2^24.
"""
from __future__ import annotations

import math
import os
import re
from typing import Dict

import numpy as np

import torch

from ._lib import SEG_COUNTS
from .ops import seg_counts  # noqa: F401  (the kernel wrapper; re-exported here)

__all__ = ["CalibrationBins", "SEG_COUNTS", "SegMetrics", "calibration_from_counts", "calibration_line", "components", "counts_to_metrics", "dice_per_class", "dice_line", "lesion_scores", "lesion_scores_from_tables",
           "seg_counts", "SweepCounts", "fit_temperature", "sweep_from_counts", "sweep_line", "sweep_thresholds", "temperature_candidates",
           "temperature_search", "ScanGeometry", "image_scores", "scores_from_counts", "patient_of", "grouped", "summarize", "bootstrap_rows",
           "bootstrap_statistics", "lesion_sizes", "lesion_sizes_from_measure"]


def _div_no_nan(a: float, b: float) -> float:
    return a / b if b != 0 else 0.0


def _f1(p: float, r: float) -> float:
    """2PR/(P+R) as the drivers compute it (MainNumpy.py:121-122): NaN, not an exception, when P + R = 0."""
    return 2.0 * p * r / (p + r) if p + r != 0 else float("nan")


def counts_to_metrics(counts, num_classes: int = 3) -> Dict[str, float]:
    """Counter buffer (``USSEG_SEG_COUNTS`` int64, CPU or device) -> ``precision, recall, f1, c2_precision, c2_recall, c2_f1,
    mean_iou`` with Keras semantics: Precision / Recall = div_no_nan; MeanIoU = the mean of IoU over the classes whose
    row + column - diagonal is non-zero (0 when there is none).  Raises ``ValueError`` when the kernel counted invalid elements
    (a class outside [0, num_classes) or a prediction outside [0, 1]: TF raises for both)."""
    nc = int(num_classes)
    if not 1 <= nc <= 4:
        raise ValueError(f"num_classes must be 1..4, got {nc}")
    c = [int(v) for v in torch.as_tensor(counts).reshape(-1)[:SEG_COUNTS].cpu().tolist()]
    invalid = c[6 + nc * nc]
    if invalid:
        raise ValueError(f"{invalid} invalid elements: a class outside [0, {nc}) or a prediction outside [0, 1] (TF raises for both)")
    tp, fp, fn, tp2, fp2, fn2 = c[:6]
    cm = [c[6 + i * nc:6 + (i + 1) * nc] for i in range(nc)]          # cm[true][pred]
    p, r = _div_no_nan(tp, tp + fp), _div_no_nan(tp, tp + fn)
    p2, r2 = _div_no_nan(tp2, tp2 + fp2), _div_no_nan(tp2, tp2 + fn2)
    iou, valid = 0.0, 0
    for k in range(nc):
        denom = sum(cm[k]) + sum(row[k] for row in cm) - cm[k][k]
        if denom != 0:
            iou += cm[k][k] / denom
            valid += 1
    return {"precision": p, "recall": r, "f1": _f1(p, r), "c2_precision": p2, "c2_recall": r2, "c2_f1": _f1(p2, r2),
            "mean_iou": _div_no_nan(iou, valid)}


def dice_per_class(counts, num_classes: int = 3):
    """Counter buffer -> the (hard) Dice score of every class from the confusion matrix the counters already hold:
    ``2*cm[c][c] / (row_c + col_c)``, div_no_nan (0.0 for a class that neither occurs nor is predicted).  Entry 2 is the class-2 (bleed)
    score the ``c2`` pair of the reference does not give (that pair is the last image column, see above).  Same ``ValueError`` as
    ``counts_to_metrics`` for invalid elements."""
    nc = int(num_classes)
    if not 1 <= nc <= 4:
        raise ValueError(f"num_classes must be 1..4, got {nc}")
    c = [int(v) for v in torch.as_tensor(counts).reshape(-1)[:SEG_COUNTS].cpu().tolist()]
    invalid = c[6 + nc * nc]
    if invalid:
        raise ValueError(f"{invalid} invalid elements: a class outside [0, {nc}) or a prediction outside [0, 1] (TF raises for both)")
    cm = [c[6 + i * nc:6 + (i + 1) * nc] for i in range(nc)]          # cm[true][pred]
    return [_div_no_nan(2.0 * cm[k][k], sum(cm[k]) + sum(row[k] for row in cm)) for k in range(nc)]


def surface_scores_from_counters(counters, sums):
    """``usseg_surface_dist``'s per-image results -> {"hd", "assd", "n_a", "n_b", "max_ab", "max_ba", "sum_ab", "sum_ba"}, NumPy arrays [N].
    hd = sqrt(max(max_ab, max_ba)) (the maxima are SQUARED distances); assd = the mean of the two directional means sum_ab / n_a and
    sum_ba / n_b, as medpy's ``assd``; both NaN for an image where either surface is empty."""
    c = torch.as_tensor(counters).cpu().numpy().astype(np.int64).reshape(-1, 4)
    s = torch.as_tensor(sums).cpu().numpy().astype(np.float64).reshape(-1, 2)
    ok = (c[:, 0] > 0) & (c[:, 1] > 0)
    na, nb = np.where(ok, c[:, 0], 1), np.where(ok, c[:, 1], 1)
    hd = np.where(ok, np.sqrt(np.maximum(np.maximum(c[:, 2], c[:, 3]), 0).astype(np.float64)), np.nan)
    assd = np.where(ok, 0.5 * (s[:, 0] / na + s[:, 1] / nb), np.nan)
    return {"hd": hd, "assd": assd, "n_a": c[:, 0], "n_b": c[:, 1], "max_ab": c[:, 2], "max_ba": c[:, 3], "sum_ab": s[:, 0], "sum_ba": s[:, 1]}


def tolerance_squared(tau) -> int:
    """The largest integer t2 whose square root - the fp64 value ``math.sqrt(t2)``, the distance as it is reported - is <= ``tau`` (>= 0,
    finite), so that ``d <= tau`` is exactly ``d2 <= t2`` for a distance d = sqrt(d2).  Integer arithmetic: floor of the square of the exact
    binary value of ``tau``, as a fraction; one more when the next integer's root ROUNDS to ``tau`` or below (tau = math.sqrt(2.0) lies below
    the real root of 2 and still admits the pixel at distance math.sqrt(2.0): t2 = 2)."""
    tau = float(tau)
    if not (math.isfinite(tau) and tau >= 0.0):
        raise ValueError(f"a surface tolerance must be finite and >= 0, got {tau}")
    num, den = tau.as_integer_ratio()                       # tau == num / den exactly
    t2 = (num * num) // (den * den)                         # floor(tau^2): the real root of m is <= tau  <=>  m <= floor(tau^2)
    assert t2 * den * den <= num * num < (t2 + 1) * den * den and math.isqrt(t2) <= tau < math.isqrt(t2) + 1
    if t2 < 2 ** 53 and math.sqrt(t2 + 1) <= tau:          # (the root of t2 + 2 is a whole step further: never again)
        t2 += 1
    if t2 >= 2 ** 31:
        raise ValueError(f"a surface tolerance of {tau} pixels is beyond any image (its square must stay below 2^31)")
    return t2


def _percentile_list(percentiles):
    qs = [float(q) for q in (percentiles if percentiles is not None else ())]
    if len(qs) > 4 or not all(math.isfinite(q) and 0.0 <= q <= 100.0 for q in qs):
        raise ValueError(f"at most 4 surface percentiles, each in [0, 100], got {qs}")
    return qs


def _tolerance_list(tolerances):
    ts = [float(t) for t in (tolerances if tolerances is not None else ())]
    if len(ts) > 4:
        raise ValueError(f"at most 4 surface tolerances, got {ts}")
    return ts, [tolerance_squared(t) for t in ts]


def _order_statistic(q, n, d2_k, d2_k1):
    """usseg.h's rule for one set of n >= 1 squared distances: pos = q / 100 * (n - 1), g = pos - floor(pos), lerp of the two roots."""
    pos = q / 100 * (n - 1)
    g = pos - math.floor(pos)
    lo, hi = math.sqrt(d2_k), math.sqrt(d2_k1)
    return lo + (hi - lo) * g


def surface_scores_from_stats(counters, sums, sel, within, percentiles=(), tolerances=()):
    """``usseg_surface_stats``' per-image results -> the dict of ``surface_scores_from_counters`` plus ``hd_pct`` [N,P] (the percentiles of
    the POOLED distances of both directions: medpy's ``hd95`` at q = 95), ``hd_pct_directed`` [N,P] (the larger of the two directions'
    percentiles: MONAI's), ``nsd`` [N,T] (surface Dice at each tolerance, pixel-count form), ``percentiles``, ``tolerances``, and the raw
    integers ``sel`` [N,3,P,2] / ``within`` [N,T,2].  The host arithmetic of usseg.h's definitions, in Python floats: percentiles NaN where
    either surface is empty; nsd NaN where both are, 0.0 where exactly one is."""
    qs = _percentile_list(percentiles)
    ts, _ = _tolerance_list(tolerances)
    out = surface_scores_from_counters(counters, sums)
    N, P, T = out["n_a"].shape[0], len(qs), len(ts)
    sel = torch.as_tensor(sel).cpu().numpy().astype(np.int64).reshape(N, 3, P, 2)
    within = torch.as_tensor(within).cpu().numpy().astype(np.int64).reshape(N, T, 2)
    pooled, directed, nsd = np.full((N, P), np.nan), np.full((N, P), np.nan), np.full((N, T), np.nan)
    for i in range(N):
        na, nb = int(out["n_a"][i]), int(out["n_b"][i])
        if na > 0 and nb > 0:
            for p, q in enumerate(qs):
                v = [_order_statistic(q, n, int(sel[i, s, p, 0]), int(sel[i, s, p, 1])) for s, n in enumerate((na, nb, na + nb))]
                pooled[i, p], directed[i, p] = v[2], max(v[0], v[1])
        if na + nb > 0:
            for t in range(T):
                nsd[i, t] = (int(within[i, t, 0]) + int(within[i, t, 1])) / (na + nb)
    out.update(hd_pct=pooled, hd_pct_directed=directed, nsd=nsd, percentiles=qs, tolerances=ts, sel=sel, within=within)
    return out


def surface_distances(a, b, device=None, *, percentiles=None, tolerances=None):
    """Hausdorff distance and average symmetric surface distance of two stacks of masks [N,H,W] (anything ``!= 0`` is inside; NumPy or
    torch), in pixels, on the device: surfaces by the 4-neighbour erosion rule, exact Euclidean distances (usseg.h ``usseg_surface_dist``).
    -> the dict of ``surface_scores_from_counters``.  With ``percentiles`` (up to 4, in [0, 100]: 95 for HD95) and / or ``tolerances`` (up to
    4, in pixels) one ``usseg_surface_stats`` call instead -> the dict of ``surface_scores_from_stats``."""
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    ta, tb = ((torch.as_tensor(m) != 0).to(device=dev, dtype=torch.uint8).contiguous() for m in (a, b))
    if ta.dim() != 3 or ta.shape != tb.shape:
        raise ValueError(f"surface_distances: two [N,H,W] stacks of one shape, got {tuple(ta.shape)} and {tuple(tb.shape)}")
    if percentiles is None and tolerances is None:
        counters, sums = ops.surface_dist(ta, tb)
        return surface_scores_from_counters(counters, sums)
    qs = _percentile_list(percentiles)
    ts, t2 = _tolerance_list(tolerances)
    counters, sums, sel, within = ops.surface_stats(ta, tb, qs, t2)
    return surface_scores_from_stats(counters, sums, sel, within, qs, ts)


def _mask_stack(m, dev, what):
    t = (torch.as_tensor(m) != 0).to(device=dev, dtype=torch.uint8).contiguous()
    if t.dim() != 3:
        raise ValueError(f"{what}: an [N,H,W] stack of masks, got {tuple(t.shape)}")
    return t


def components(mask, connectivity=8, prob=None, device=None):
    """Connected components of a stack of masks [N,H,W] (anything ``!= 0`` is inside; NumPy or torch) on the device (usseg.h
    ``usseg_label_components`` / ``usseg_component_stats``): -> {"labels" int32 [N,H,W], "count" [N], "area" [N,cap], "bbox" [N,cap,4]
    (y_min, x_min, y_max, x_max), "centroid" fp64 [N,cap,2] (y, x; exact integer sums divided once), "peak" fp32 [N,cap]}, NumPy arrays with
    cap = max(count): the counts are read back once, then the table is sized.  Rows past an image's count are zero (centroid NaN).
    ``prob`` [N,H,W] gives each component's peak probability (0 without it)."""
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    tm = _mask_stack(mask, dev, "components")
    tp = None
    if prob is not None:
        tp = torch.as_tensor(prob).to(device=dev, dtype=torch.float32).contiguous()
        if tp.shape != tm.shape:
            raise ValueError(f"components: prob {tuple(tp.shape)} and mask {tuple(tm.shape)} differ in shape")
    labels, count = ops.label_components(tm, connectivity)
    count = count.cpu().numpy().astype(np.int64)
    cap = int(count.max()) if count.size else 0
    st = ops.component_stats(labels, cap, tp).cpu().numpy()
    area = st[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        centroid = st[..., 5:7].astype(np.float64) / area[..., None]
    peak = st[..., 7].astype(np.uint32).view(np.float32) if st.size else np.zeros(st.shape[:2], np.float32)
    return {"labels": labels.cpu().numpy(), "count": count, "area": area, "bbox": st[..., 1:5], "centroid": centroid, "peak": peak}


def lesion_scores_from_tables(count_true, count_pred, hit_true, hit_pred, area_true, area_pred, min_overlap=1):
    """The lesion-wise scores from the integer tables of one stack: ``count_*`` [N] component counts, ``hit_true`` [N,cap_t] the pixels of each
    labelled lesion inside the prediction, ``hit_pred`` [N,cap_p] the pixels of each predicted component inside the label, ``area_*`` the
    component areas (columns past an image's count are ignored).  A lesion is detected with at least ``min_overlap`` of its pixels inside the
    prediction; a predicted component without a pixel inside the label is a false positive.  -> per image (int64 [N]) ``n_true, n_pred,
    detected, missed, false_pos, largest_true, largest_pred`` and over the stack ``sensitivity`` = detected / n_true, ``precision`` =
    (n_pred - false_pos) / n_pred, their ``f1`` and ``fp_per_image`` = false_pos / N (every division div_no_nan)."""
    if int(min_overlap) < 1:
        raise ValueError(f"min_overlap must be >= 1, got {min_overlap}")
    nt, npd = np.asarray(count_true, np.int64).reshape(-1), np.asarray(count_pred, np.int64).reshape(-1)
    N = nt.shape[0]
    table = lambda t: (lambda a: a.reshape(N, a.size // N if N else 0))(np.asarray(t, np.int64))
    ht, hp, at, apd = table(hit_true), table(hit_pred), table(area_true), table(area_pred)
    if npd.shape[0] != N or (N and (ht.shape[1] < nt.max() or hp.shape[1] < npd.max() or at.shape[1] < nt.max() or apd.shape[1] < npd.max())):
        raise ValueError("lesion_scores_from_tables: a table is narrower than the largest count")
    vt = np.arange(ht.shape[1])[None, :] < nt[:, None]
    vp = np.arange(hp.shape[1])[None, :] < npd[:, None]
    detected = ((ht >= int(min_overlap)) & vt).sum(1)
    false_pos = ((hp == 0) & vp).sum(1)
    largest_t = np.where(np.arange(at.shape[1])[None, :] < nt[:, None], at, 0).max(1, initial=0)
    largest_p = np.where(np.arange(apd.shape[1])[None, :] < npd[:, None], apd, 0).max(1, initial=0)
    sens = _div_no_nan(float(detected.sum()), float(nt.sum()))
    prec = _div_no_nan(float(npd.sum() - false_pos.sum()), float(npd.sum()))
    return {"n_true": nt, "n_pred": npd, "detected": detected, "missed": nt - detected, "false_pos": false_pos, "largest_true": largest_t,
            "largest_pred": largest_p, "sensitivity": sens, "precision": prec, "f1": _div_no_nan(2.0 * prec * sens, prec + sens),
            "fp_per_image": _div_no_nan(float(false_pos.sum()), float(N))}


def lesion_scores(pred, true, *, connectivity=8, min_overlap=1, device=None):
    """Lesion-wise detection scores of two stacks of masks [N,H,W] on the device: both are labelled (``usseg_label_components``), the
    overlap and area tables are built there (``usseg_component_overlap`` / ``usseg_component_stats``), and ``lesion_scores_from_tables`` turns
    them into numbers.  One read-back of the counts sizes the tables."""
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    tp, tt = _mask_stack(pred, dev, "lesion_scores"), _mask_stack(true, dev, "lesion_scores")
    if tp.shape != tt.shape:
        raise ValueError(f"lesion_scores: two [N,H,W] stacks of one shape, got {tuple(tp.shape)} and {tuple(tt.shape)}")
    N, H, W = tp.shape
    ws = torch.empty(max(ops.components_ws_bytes(N, H, W), 16), dtype=torch.uint8, device=dev)
    lp, cp = ops.label_components(tp, connectivity, ws=ws)
    lt, ct = ops.label_components(tt, connectivity, ws=ws)
    counts = torch.stack([ct, cp]).cpu().numpy().astype(np.int64)
    cap_t, cap_p = (int(counts[0].max()), int(counts[1].max())) if N else (0, 0)
    hit_t, hit_p = ops.component_overlap(lt, lp, cap_t, cap_p)
    area_t, area_p = ops.component_stats(lt, cap_t)[..., 0], ops.component_stats(lp, cap_p)[..., 0]
    return lesion_scores_from_tables(counts[0], counts[1], hit_t.cpu().numpy(), hit_p.cpu().numpy(), area_t.cpu().numpy(), area_p.cpu().numpy(),
                                     min_overlap)


def dice_line(neuralnet, seg_metrics):
    """The drivers' extra report line: the per-class Dice list when the model trains with a region-overlap, the Lovasz-softmax or a top-k loss, else None
    (nothing is printed); the history keeps its keys either way."""
    if all(getattr(neuralnet, name, None) is None for name in ("overlap_loss", "lovasz_loss", "topk_loss")):      # (Arch A has none of the properties)
        return None
    return seg_metrics.dice()


class SegMetrics:
    """The drivers' five Keras metric objects as ONE counter buffer: ``update_state`` is one launch, ``result`` one copy to the
    host, ``reset_states`` one fill.  ``round=True`` is the MainNumpy / TBI_TransUNet / MainParallel scoring (tf.math.round of
    labels and probabilities first); ``round=False`` is TBI_ResNest.test's, which passes them unrounded (TBI_ResNest.py:423-426).
    Update tensors must live on the device: there is no CPU fallback."""

    def __init__(self, num_classes: int = 3, round: bool = True, device=None):
        if not 1 <= int(num_classes) <= 4:
            raise ValueError(f"num_classes must be 1..4, got {num_classes}")
        self.num_classes, self.round = int(num_classes), bool(round)
        self.counts = torch.zeros(SEG_COUNTS, dtype=torch.int64, device=device if device is not None else "cuda")

    def update_state(self, y_true: torch.Tensor, probs: torch.Tensor) -> None:
        """Add one batch, fp32 [B,H,W,C] on the counters' device; enqueued on the current stream (no host synchronisation)."""
        seg_counts(y_true, probs, self.counts, self.round, self.num_classes)

    def reduce(self, group=None) -> None:
        """SUM all-reduce of the counters over the replicas of ``group`` (replaces MirroredStrategy.reduce / gather of the
        probabilities and labels, MainParallel.py:148-176).  Exact; call once before ``result()``."""
        import torch.distributed as dist
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def result(self) -> Dict[str, float]:
        return counts_to_metrics(self.counts.cpu(), self.num_classes)

    def dice(self):
        """Per-class Dice of the counters so far (``dice_per_class``); call after ``reduce`` under data parallelism."""
        return dice_per_class(self.counts.cpu(), self.num_classes)

    def reset_states(self) -> None:
        self.counts.zero_()


# ---------------------------------------------------------------------------------------------------------- calibration
def calibration_from_counts(counts) -> Dict[str, object]:
    """Counter block of ``usseg_calibration_bins`` (int64 [bins*3 + 2], CPU or device) -> the reliability table and its scores, in fp64:
    ``n``, ``accuracy``, ``confidence`` per bin (0 in an empty bin), ``ece`` = sum_b n_b/N * |acc_b - conf_b| (the expected calibration error of
    Guo et al., ICML 2017), ``mce`` = the largest gap over the non-empty bins, ``brier`` = the mean over the valid pixels of
    sum_c (p_c - onehot_c)^2, and ``n_invalid``.  The three scores are NaN when no pixel was valid."""
    c = np.asarray(torch.as_tensor(counts).reshape(-1).cpu().numpy(), np.int64)
    if c.size < 5 or (c.size - 2) % 3:
        raise ValueError(f"a calibration counter block holds bins*3 + 2 integers, got {c.size}")
    bins = (c.size - 2) // 3
    t = c[:bins * 3].reshape(bins, 3).astype(np.float64)
    n = t[:, 0]
    N = float(n.sum())
    full = n > 0
    acc = np.divide(t[:, 1], n, out=np.zeros(bins), where=full)
    conf = np.divide(t[:, 2] / 2.0 ** 24, n, out=np.zeros(bins), where=full)
    gap = np.abs(acc - conf)
    out = dict(n=c[:bins * 3].reshape(bins, 3)[:, 0].copy(), accuracy=acc, confidence=conf, n_invalid=int(c[bins * 3 + 1]))
    if N > 0:
        out.update(ece=float((n / N * gap).sum()), mce=float(gap[full].max()), brier=float(c[bins * 3]) / 2.0 ** 24 / N)
    else:
        out.update(ece=float("nan"), mce=float("nan"), brier=float("nan"))
    return out


class CalibrationBins:
    """Reliability counters that stay on the device, after ``SegMetrics``: ``update`` is one launch (``ops.calibration_bins``), ``result`` the one
    copy to the host, ``reset`` one fill.  ``cls`` -1 is top-label calibration, k the class-wise calibration of class k."""

    def __init__(self, bins: int = 15, cls: int = -1, device=None):
        from ._lib import CALIB_MAX_BINS
        bins, cls = int(bins), int(cls)
        if not 1 <= bins <= CALIB_MAX_BINS:
            raise ValueError(f"bins must be 1..{CALIB_MAX_BINS}, got {bins}")
        if not -1 <= cls <= 3:
            raise ValueError(f"cls must be -1 (top label) or a class 0..3, got {cls}")
        self.bins, self.cls = bins, cls
        self.counts = torch.zeros(bins * 3 + 2, dtype=torch.int64, device=device if device is not None else "cuda")

    def update(self, probs: torch.Tensor, y: torch.Tensor) -> None:
        """Add one batch, fp32 [B,H,W,C] on the counters' device; enqueued on the current stream (no host synchronisation)."""
        from .ops import calibration_bins
        calibration_bins(probs, y, self.counts, self.bins, self.cls)

    def result(self) -> Dict[str, object]:
        return calibration_from_counts(self.counts.cpu())

    def reset(self) -> None:
        self.counts.zero_()


def calibration_line(r) -> str:
    """The drivers' one line per epoch for ``calibration_from_counts``' dict."""
    return "calibration: ECE = {:.5f}, MCE = {:.5f}, Brier = {:.5f}, invalid = {}".format(r["ece"], r["mce"], r["brier"], r["n_invalid"])


# ---------------------------------------------------------------------------------------------------------- operating points
def sweep_thresholds(bins: int) -> np.ndarray:
    """fp32 [bins + 1]: ``threshold[k]`` such that "bin >= k" is ``s > threshold[k]`` for every valid fp32 score s.  ``bins`` is a power of two, so
    k/bins and s*bins are exact: bin >= k is s >= k/bins, and the largest fp32 below k/bins turns that into a strict comparison, the form every
    ``threshold=`` argument of the evaluator takes.  k = 0 is -inf (everything is predicted positive); k = bins is 1.0 (nothing is: s = 1 lies
    in the LAST bin, so the largest fp32 below 1 would wrongly let it through)."""
    bins = int(bins)
    t = np.empty(bins + 1, np.float32)
    t[0] = -np.inf
    t[1:] = np.nextafter((np.arange(1, bins + 1, dtype=np.float64) / bins).astype(np.float32), np.float32(0))
    t[bins] = 1.0
    return t


def sweep_from_counts(counts) -> Dict[str, object]:
    """Counter block of ``usseg_score_sweep`` (int64 [2*bins + 1], CPU or device) -> the operating points of the swept class, from Python
    integers and fp64 on the host.  Operating point k = 0..bins predicts positive iff bin >= k (``threshold[k]``: ``sweep_thresholds``):
    ``tp, fp, fn, tn`` (int64 [bins+1]), ``tpr``, ``fpr`` (NaN without positives / negatives), ``precision`` (1 where tp + fp = 0), ``dice`` =
    2tp/(2tp+fp+fn) (0 where that is 0/0).  ``auc``: the exact Mann-Whitney statistic of the binned score, ties at one half,
    sum_b pos_b*(2*neg_below_b + neg_b) / (2*P*N), NaN when P or N is 0.  ``average_precision``: sum_k (recall_k - recall_(k+1)) * precision_k,
    NaN when P is 0.  ``best_dice`` and ``best_youden`` (tpr - fpr): (k, threshold, value), ties to the smallest k.  ``n_invalid``."""
    c = [int(v) for v in torch.as_tensor(counts).reshape(-1).cpu().tolist()]
    bins = (len(c) - 1) // 2
    if len(c) < 5 or len(c) != 2 * bins + 1 or bins & (bins - 1):
        raise ValueError(f"a sweep counter block holds 2*bins + 1 integers with bins a power of two, got {len(c)}")
    neg, pos = c[0:2 * bins:2], c[1:2 * bins:2]
    P, N = sum(pos), sum(neg)
    tp, fp = [0] * (bins + 1), [0] * (bins + 1)
    for k in range(bins - 1, -1, -1):
        tp[k] = tp[k + 1] + pos[k]
        fp[k] = fp[k + 1] + neg[k]
    fn, tn = [P - v for v in tp], [N - v for v in fp]
    nan = float("nan")
    tpr = [v / P if P else nan for v in tp]
    fpr = [v / N if N else nan for v in fp]
    precision = [tp[k] / (tp[k] + fp[k]) if tp[k] + fp[k] else 1.0 for k in range(bins + 1)]
    dice = [2 * tp[k] / (2 * tp[k] + fp[k] + fn[k]) if 2 * tp[k] + fp[k] + fn[k] else 0.0 for k in range(bins + 1)]
    below, num = 0, 0
    for b in range(bins):
        num += pos[b] * (2 * below + neg[b])
        below += neg[b]
    auc = num / (2 * P * N) if P and N else nan
    ap = sum((tp[k] - tp[k + 1]) * precision[k] for k in range(bins)) / P if P else nan
    thr = sweep_thresholds(bins)

    def best(v):
        k = max(range(bins + 1), key=lambda i: (v[i], -i)) if not any(math.isnan(x) for x in v) else 0
        return k, float(thr[k]), float(v[k])
    return dict(tp=np.array(tp, np.int64), fp=np.array(fp, np.int64), fn=np.array(fn, np.int64), tn=np.array(tn, np.int64),
                tpr=np.array(tpr), fpr=np.array(fpr), precision=np.array(precision), dice=np.array(dice), threshold=thr, auc=auc,
                average_precision=ap, best_dice=best(dice), best_youden=best([a - b for a, b in zip(tpr, fpr)]), n_invalid=c[2 * bins])


class SweepCounts:
    """Sweep counters that stay on the device, after ``CalibrationBins``: ``update`` is one launch (``ops.score_sweep``), ``result`` the one copy
    to the host (-> ``sweep_from_counts``' dict), ``reset`` one fill.  ``cls``: the swept class; negative counts from the last class."""

    def __init__(self, bins: int = 1024, cls: int = -1, device=None):
        from ._lib import SWEEP_MAX_BINS
        bins, cls = int(bins), int(cls)
        if not 2 <= bins <= SWEEP_MAX_BINS or bins & (bins - 1):
            raise ValueError(f"bins must be a power of two in 2..{SWEEP_MAX_BINS}, got {bins}")
        if not -4 <= cls <= 3:
            raise ValueError(f"cls must be a class 0..3 (or negative, from the last), got {cls}")
        self.bins, self.cls = bins, cls
        self.counts = torch.zeros(2 * bins + 1, dtype=torch.int64, device=device if device is not None else "cuda")

    def update(self, probs: torch.Tensor, y: torch.Tensor) -> None:
        """Add one batch, fp32 [B,H,W,C] on the counters' device; enqueued on the current stream (no host synchronisation)."""
        from .ops import score_sweep
        score_sweep(probs, y, self.counts, self.bins, self.cls)

    def result(self) -> Dict[str, object]:
        return sweep_from_counts(self.counts.cpu())

    def reset(self) -> None:
        self.counts.zero_()


def sweep_line(r) -> str:
    """The drivers' one line per epoch for ``sweep_from_counts``' dict."""
    return "sweep: AUC = {:.5f}, AP = {:.5f}, best Dice = {:.5f} at threshold {:.6f}, invalid = {}".format(
        r["auc"], r["average_precision"], r["best_dice"][2], r["best_dice"][1], r["n_invalid"])


def _f32(v) -> float:
    return float(np.float32(v))


def temperature_candidates(lo: float, hi: float, n: int, geometric: bool):
    """The n candidates of one round of ``fit_temperature`` on [lo, hi], rounded to fp32 (the values the kernel sees), ascending."""
    if n == 1:
        return [_f32(lo)]
    if geometric:
        return [_f32(lo * (hi / lo) ** (i / (n - 1))) for i in range(n)]
    return [_f32(lo + (hi - lo) * (i / (n - 1))) for i in range(n)]


def temperature_search(evaluate, *, lo=1 / 8, hi=8.0, candidates=16, rounds=4):
    """The bracket search of ``fit_temperature`` over ``evaluate(betas) -> [sum_0, ..., sum_(n-1), n_valid, n_invalid]`` (integers).  Round 0:
    ``candidates`` betas geometrically spaced on [lo, hi]; each later round: ``candidates`` betas evenly spaced on [the neighbour below the
    arg-min, the neighbour above it] (the arg-min itself at an end of the list).  Ties go to the smallest beta.  The NLL is convex in beta
    (a log-sum-exp of linear functions minus a linear one), so the bracket keeps the minimiser.  Last, beta = 1 is evaluated on its own and wins
    when its sum is strictly smaller (so the result is never worse than no scaling).  -> (beta, its sum, the sum at 1, (bracket lo, bracket hi),
    n_valid, n_invalid)."""
    candidates, rounds = int(candidates), int(rounds)
    if not (0.0 < lo < hi <= 16.0):
        raise ValueError(f"fit_temperature: 0 < lo < hi <= 16, got [{lo}, {hi}]")
    if not 3 <= candidates <= 16 or rounds < 1:
        raise ValueError(f"fit_temperature: 3..16 candidates and at least one round, got {candidates} and {rounds}")
    a, b = float(lo), float(hi)
    for r in range(rounds):
        betas = temperature_candidates(a, b, candidates, geometric=r == 0)
        c = [int(v) for v in evaluate(betas)]
        sums = c[:len(betas)]
        i = min(range(len(betas)), key=lambda j: (sums[j], betas[j]))
        if r == 0 and i in (0, len(betas) - 1):
            edge = "lower" if i == 0 else "upper"
            raise ValueError(f"fit_temperature: the smallest NLL lies on the {edge} edge of [{lo}, {hi}] (beta = {betas[i]}): widen the interval")
        a, b = betas[max(i - 1, 0)], betas[min(i + 1, len(betas) - 1)]
        beta, best, n, n_invalid = betas[i], sums[i], c[len(betas)], c[len(betas) + 1]
        if not a < b:
            break                                        # the bracket has closed to neighbouring fp32 values
    at1 = int(evaluate([1.0])[0])
    if at1 < best:                                       # the candidates straddle 1 without holding it: "no scaling" is then the better answer
        beta, best = 1.0, at1
    return beta, best, at1, (a, b), n, n_invalid


def fit_temperature(batches, *, lo=1 / 8, hi=8.0, candidates=16, rounds=4, device=None) -> Dict[str, object]:
    """Temperature scaling (Guo et al., ICML 2017) fitted on the device: the beta = 1/T that minimises the negative log-likelihood of the labels
    under softmax(beta * log(probs + 1e-7)), by ``temperature_search``.  ``batches``: a re-iterable of (probs, y_true) pairs [B,H,W,C], device
    tensors or numpy arrays (uploaded per round).  Each round is one ``ops.temperature_nll`` launch per batch - every candidate in one read -
    and ONE read-back.  The sums are integers: the fit is bitwise reproducible.  An arg-min on the edge of [lo, hi] after round 0 raises a
    ``ValueError`` naming the edge.  -> dict(beta, temperature = 1/beta, nll and nll_at_1 (means over the valid pixels), bracket, n, n_invalid)."""
    from ._lib import TEMP_NLL_UNIT
    from .ops import temperature_nll
    dev = torch.device(device if device is not None else "cuda")

    def on_dev(t):
        return torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32) if isinstance(t, np.ndarray) else t).to(device=dev, dtype=torch.float32).contiguous()

    def evaluate(betas):
        counts = torch.zeros(len(betas) + 2, dtype=torch.int64, device=dev)
        for probs, y in batches:
            temperature_nll(on_dev(probs), on_dev(y), betas, counts)
        return counts.cpu().tolist()                     # the ONE read-back of the round
    beta, best, at1, bracket, n, n_invalid = temperature_search(evaluate, lo=lo, hi=hi, candidates=candidates, rounds=rounds)
    per = TEMP_NLL_UNIT / n if n else float("nan")
    return dict(beta=beta, temperature=1.0 / beta, nll=best * per, nll_at_1=at1 * per, bracket=bracket, n=n, n_invalid=n_invalid)


# ---- per-image and per-patient scores, bleed sizes in physical units (csrc/scores.hip, include/usseg_scores.h) ----------------------------
class ScanGeometry:
    """The physical geometry of the polar grid, for MEASURING (``TBIEvaluator.ConeGeometry`` is the one that draws): ``xAxis``, ``yAxis`` [H,W],
    finite, H, W >= 2 (``axis/xAxis.npy`` / ``axis/yAxis.npy``, the position of every sample in axis units).  The axes are used as they are:
    the ``astype(int)`` the reference applies before it draws (TBIEvaluator.py:23-24) is a display quirk - it only snaps the figure's
    vertices to whole units - and would put the areas below off by up to a whole cell.

    ``area`` fp64 [H,W]: the cell around each sample, |dXi*dYj - dXj*dYi| (the Jacobian of (row, column) -> (x, y)), where d.i is the central
    difference along rows, (v[i+1,j] - v[i-1,j]) * 0.5, one-sided in the first and last row (v[1] - v[0], v[H-1] - v[H-2]), and d.j the same
    along columns.  A deep pixel of a sector scan covers many times the area of a shallow one: a pixel count is not the size of a bleed.

    Fixed-point tables for the kernels (include/usseg_scores.h states the overflow argument: 2^20 * 2^16 * 2^26 = 2^62):
        quantum = area.max() / (2^20 - 1)         wq = rint(area / quantum), uint32, every value < 2^20
        xstep = (X.max() - X.min()) / (2^16 - 1)  xq = rint((X - X.min()) / xstep), int32 in [0, 65535]; a zero span: xstep = 1, xq = 0
    and ystep / yq alike.  ``area_of``, ``x_of`` and ``y_of`` convert the kernels' integer sums back to axis units.  Bounds: every cell is
    rounded to the nearest quantum once, so an area summed over n pixels is off by at most n * quantum / 2; every coordinate is rounded to
    the nearest step once, so a centroid is within xstep / 2 (ystep / 2) of the centroid of the exact coordinates under the same weights,
    and an extent within xstep / 2 of the exact one.  A grid whose largest area is 0 or not finite (collapsed, or overflowing) is refused."""

    WQ_MAX, Q_MAX, MAX_DIM = 2 ** 20 - 1, 2 ** 16 - 1, 8192

    def __init__(self, xAxis, yAxis):
        X, Y = np.asarray(xAxis), np.asarray(yAxis)
        if X.shape != Y.shape or X.ndim != 2 or min(X.shape) < 2:
            raise ValueError(f"xAxis {X.shape} and yAxis {Y.shape} must be one [H,W] grid with H, W >= 2")
        if max(X.shape) > self.MAX_DIM:
            raise ValueError(f"H and W must not exceed {self.MAX_DIM} (the kernels' limit, on which the int64 budget rests), got {X.shape}")
        if not (np.issubdtype(X.dtype, np.number) and np.issubdtype(Y.dtype, np.number)) or np.iscomplexobj(X) or np.iscomplexobj(Y):
            raise ValueError("xAxis and yAxis must hold real numbers")
        X, Y = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(Y, np.float64)
        if not (np.isfinite(X).all() and np.isfinite(Y).all()):
            raise ValueError("xAxis and yAxis must hold finite numbers")

        def d_i(v):
            d = np.empty_like(v)
            d[1:-1] = (v[2:] - v[:-2]) * 0.5
            d[0] = v[1] - v[0]
            d[-1] = v[-1] - v[-2]
            return d

        def d_j(v):
            d = np.empty_like(v)
            d[:, 1:-1] = (v[:, 2:] - v[:, :-2]) * 0.5
            d[:, 0] = v[:, 1] - v[:, 0]
            d[:, -1] = v[:, -1] - v[:, -2]
            return d
        with np.errstate(over="ignore", invalid="ignore"):
            area = np.abs(d_i(X) * d_j(Y) - d_j(X) * d_i(Y))
        top = float(area.max())
        if not (np.isfinite(area).all() and top > 0.0):
            raise ValueError(f"the grid spans no area, or one that is not finite (largest cell {top!r})")
        self.X, self.Y, self.area, self.grid = X, Y, area, X.shape
        self.quantum = top / self.WQ_MAX
        self.wq = np.minimum(np.rint(area / self.quantum), self.WQ_MAX).astype(np.uint32)
        self.x_min, self.xstep, self.xq = self._quantise(X)
        self.y_min, self.ystep, self.yq = self._quantise(Y)
        self._dev = {}

    @classmethod
    def _quantise(cls, V):
        lo = float(V.min())
        span = float(V.max()) - lo
        if not np.isfinite(span):
            raise ValueError(f"the axis spans {span!r}: not a finite number")
        step = span / cls.Q_MAX
        if not step > 0.0:                                                  # a zero span (or one so small that the step underflows)
            return lo, 1.0, np.zeros(V.shape, np.int32)
        return lo, step, np.clip(np.rint((V - lo) / step), 0, cls.Q_MAX).astype(np.int32)

    @classmethod
    def from_dir(cls, axis_dir):
        """Read ``xAxis.npy`` and ``yAxis.npy`` (``DataFilePlayGround.FetchPolarAxis``'s output) from ``axis_dir``, uncast."""
        return cls(np.load(os.path.join(axis_dir, "xAxis.npy")), np.load(os.path.join(axis_dir, "yAxis.npy")))

    def tables(self, device):
        """(wq, xq, yq) as int32 [H,W] tensors on ``device`` (wq < 2^20 reads the same as uint32), uploaded once per device."""
        dev = torch.device(device)
        if dev not in self._dev:
            self._dev[dev] = tuple(torch.from_numpy(np.ascontiguousarray(t.astype(np.int32))).to(dev) for t in (self.wq, self.xq, self.yq))
        return self._dev[dev]

    def area_of(self, sum_wq):
        """A sum of ``wq`` -> area in axis units^2 (off by at most n * quantum / 2 over n pixels)."""
        return np.asarray(sum_wq, np.float64) * self.quantum

    @staticmethod
    def _centre(lo, step, sum_wq_q, sum_wq):
        with np.errstate(invalid="ignore", divide="ignore"):
            return lo + step * (np.asarray(sum_wq_q, np.float64) / np.asarray(sum_wq, np.float64))

    def x_of(self, sum_wxq, sum_wq):
        """Sums of ``wq * xq`` and of ``wq`` -> the area-weighted x in axis units (NaN for an empty sum)."""
        return self._centre(self.x_min, self.xstep, sum_wxq, sum_wq)

    def y_of(self, sum_wyq, sum_wq):
        return self._centre(self.y_min, self.ystep, sum_wyq, sum_wq)

    def x_at(self, xq):
        """A quantised coordinate (an extent of ``component_measure``) -> axis units."""
        return self.x_min + self.xstep * np.asarray(xq, np.float64)

    def y_at(self, yq):
        return self.y_min + self.ystep * np.asarray(yq, np.float64)


SCORE_COUNTS = ("tp", "fp", "fn", "tn")
SCORE_AREA_COUNTS = ("w_true", "w_pred", "w_tp")          # sums of ScanGeometry.wq: integers, in quanta
SCORE_RATIOS = ("dice", "iou", "sensitivity", "precision")
SCORE_AREAS = ("area_true", "area_pred", "area_tp", "area_dice", "area_error")
DICE_FIXED_ONE = 2 ** 30                                 # a per-image Dice travels through the bootstrap as rint(dice * 2^30)


def _ratio(num, den):
    """num / den element-wise in fp64, NaN where den == 0 (an undefined score is left out of a mean, never counted as 0 or 1)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def scores_from_counts(tp, fp, fn, tn, w_true=None, w_pred=None, w_tp=None, quantum=None):
    """Integer columns -> the score table: the counts (int64), ``dice`` = 2tp / (2tp + fp + fn), ``iou`` = tp / (tp + fp + fn),
    ``sensitivity`` = tp / (tp + fn), ``precision`` = tp / (tp + fp), each NaN where its denominator is 0; with the area sums (in quanta
    of ``quantum`` axis units^2) also ``area_true / area_pred / area_tp``, ``area_dice`` = 2 w_tp / (w_true + w_pred) and ``area_error`` =
    area_pred - area_true.  Every derived column is one fp64 division (and one product) of exact integers."""
    t = {k: np.asarray(v, np.int64).reshape(-1) for k, v in zip(SCORE_COUNTS, (tp, fp, fn, tn))}
    tp_, fp_, fn_ = t["tp"], t["fp"], t["fn"]
    t["dice"] = _ratio(2 * tp_, 2 * tp_ + fp_ + fn_)
    t["iou"] = _ratio(tp_, tp_ + fp_ + fn_)
    t["sensitivity"] = _ratio(tp_, tp_ + fn_)
    t["precision"] = _ratio(tp_, tp_ + fp_)
    if w_true is not None:
        q = float(quantum)
        wt, wp, wtp = (np.asarray(v, np.int64).reshape(-1) for v in (w_true, w_pred, w_tp))
        t.update(w_true=wt, w_pred=wp, w_tp=wtp, quantum=q, area_true=wt * q, area_pred=wp * q, area_tp=wtp * q,
                 area_dice=_ratio(2 * wtp, wt + wp), area_error=(wp - wt) * q)
    return t


def image_scores(pred_mask, true_mask, geometry=None, device=None):
    """The overlap table per image of two stacks of masks [N,H,W] (anything ``!= 0`` is inside; NumPy or torch), counted on the device by
    one ``ops.image_confusion`` call and read back once -> ``scores_from_counts``' table, one entry per image.  With a ``ScanGeometry``
    every pixel also counts with the area of its cell, which gives the ``area_*`` columns in axis units^2."""
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    tp_, tt = _mask_stack(pred_mask, dev, "image_scores"), _mask_stack(true_mask, dev, "image_scores")
    if tp_.shape != tt.shape:
        raise ValueError(f"image_scores: two [N,H,W] stacks of one shape, got {tuple(tp_.shape)} and {tuple(tt.shape)}")
    weight = None
    if geometry is not None:
        if tuple(geometry.grid) != tuple(tp_.shape[1:]):
            raise ValueError(f"image_scores: the geometry is {tuple(geometry.grid)}, the masks {tuple(tp_.shape[1:])}")
        weight = geometry.tables(dev)[0]
    cm, wcm, invalid = ops.image_confusion(tp_, tt, 2, weight)
    cm = cm.cpu().numpy()                                                   # cm[n][truth][pred]
    if weight is None:
        return scores_from_counts(cm[:, 1, 1], cm[:, 0, 1], cm[:, 1, 0], cm[:, 0, 0])
    w = wcm.cpu().numpy()
    return scores_from_counts(cm[:, 1, 1], cm[:, 0, 1], cm[:, 1, 0], cm[:, 0, 0], w[:, 1, 0] + w[:, 1, 1], w[:, 0, 1] + w[:, 1, 1], w[:, 1, 1],
                              geometry.quantum)


def patient_of(name, pattern=r"DoD(\d+)"):
    """The patient of an image name: what ``pattern`` captures in it (its first group, or the whole match of a pattern without one) -
    ``DataFilePlayGround``'s patient folders are named DoD<number>.  A name that does not match is its own group."""
    if isinstance(name, bytes):
        name = name.decode("utf-8", "replace")
    name = str(name)
    m = re.search(pattern, name)
    if not m:
        return name
    return m.group(1) if m.re.groups else m.group(0)


def _group_index(groups, n):
    groups = list(groups)
    if len(groups) != n:
        raise ValueError(f"{len(groups)} group labels for {n} images")
    order = {}
    idx = np.array([order.setdefault(g, len(order)) for g in groups], np.int64).reshape(-1)
    return list(order), idx


def _sum_by(idx, n_groups, col):
    out = np.zeros(n_groups, np.int64)
    np.add.at(out, idx, np.asarray(col, np.int64))
    return out


def grouped(table, groups):
    """Sum the integer columns of a score table per group (``groups``: one label per image, e.g. ``patient_of`` of each name) and re-derive
    the ratios from the sums -> a table with one entry per group, in order of first appearance, plus ``groups`` (the labels) and
    ``n_images`` (images per group)."""
    n = len(table["tp"])
    labels, idx = _group_index(groups, n)
    cols = SCORE_COUNTS + (SCORE_AREA_COUNTS if "w_true" in table else ())
    sums = {c: _sum_by(idx, len(labels), table[c]) for c in cols}
    out = scores_from_counts(*(sums[c] for c in cols), **({"quantum": table["quantum"]} if "w_true" in table else {}))
    out["groups"], out["n_images"] = labels, _sum_by(idx, len(labels), np.ones(n, np.int64))
    return out


def _defined_stats(v):
    v = np.asarray(v, np.float64)
    d = v[~np.isnan(v)]
    return (float(d.mean()) if d.size else float("nan"), float(np.median(d)) if d.size else float("nan"), int(d.size))


def bootstrap_rows(table, groups=None):
    """The integer rows the bootstrap resamples, one per unit (a group when ``groups`` is given, else an image), and their column names:
    tp, fp, fn, dice_q = the sum of rint(dice * 2^30) over the unit's images with a defined Dice, dice_n = their number; with areas also
    w_tp, w_true, w_pred."""
    n = len(table["tp"])
    dice = np.asarray(table["dice"], np.float64)
    ok = ~np.isnan(dice)
    cols = {"tp": table["tp"], "fp": table["fp"], "fn": table["fn"],
            "dice_q": np.where(ok, np.rint(np.where(ok, dice, 0.0) * DICE_FIXED_ONE), 0).astype(np.int64), "dice_n": ok.astype(np.int64)}
    if "w_true" in table:
        cols.update(w_tp=table["w_tp"], w_true=table["w_true"], w_pred=table["w_pred"])
    names = tuple(cols)
    if groups is None:
        return names, np.stack([np.asarray(cols[c], np.int64) for c in names], 1).reshape(n, len(names))
    labels, idx = _group_index(groups, n)
    return names, np.stack([_sum_by(idx, len(labels), cols[c]) for c in names], 1).reshape(len(labels), len(names))


def bootstrap_statistics(names, sums, quantum=None):
    """Column sums (of ``bootstrap_rows``' columns; any leading shape) -> the four statistics: ``pooled_dice``, ``mean_dice``, and with areas
    ``area_dice`` and ``area_error_total`` (axis units^2); NaN where a denominator is 0."""
    s = {c: np.asarray(sums)[..., i].astype(np.int64) for i, c in enumerate(names)}
    out = {"pooled_dice": _ratio(2 * s["tp"], 2 * s["tp"] + s["fp"] + s["fn"]), "mean_dice": _ratio(s["dice_q"], s["dice_n"]) / DICE_FIXED_ONE}
    if "w_true" in s:
        out["area_dice"] = _ratio(2 * s["w_tp"], s["w_true"] + s["w_pred"])
        out["area_error_total"] = (s["w_pred"] - s["w_true"]) * float(quantum)
    return out


def summarize(table, groups=None, bootstrap=0, seed=0, alpha=0.05, device=None):
    """A score table -> its summary:
      ``pooled``        the scores of the summed counts (``scores_from_counts`` of the column sums: the run as one image);
      ``mean / median`` of every ratio over the images where it is defined, ``defined`` = how many those are (an image empty in both masks
                        has no Dice: it is left out, not counted as 0 or 1);
      ``bland_altman``  of ``area_error`` (with areas): bias = its mean, sd (n - 1), limits of agreement bias -+ 1.96 sd, n.
    ``bootstrap`` = R > 0 adds ``bootstrap``: percentile intervals [alpha/2, 1 - alpha/2] of ``bootstrap_statistics``' four statistics over R
    replicates drawn on the device (``ops.bootstrap_sums``, reproducible from ``seed``).  The resampling unit is the group when ``groups``
    is given - a cluster bootstrap over patients, whose frames are correlated - else the image.  Replicates whose statistic is NaN are
    dropped from that statistic's interval and counted in ``dropped``."""
    n = len(table["tp"])
    areas = "w_true" in table
    cols = SCORE_COUNTS + (SCORE_AREA_COUNTS if areas else ())
    pooled = scores_from_counts(*([int(np.asarray(table[c], np.int64).sum())] for c in cols), **({"quantum": table["quantum"]} if areas else {}))
    pooled = {k: (v[0].item() if isinstance(v, np.ndarray) else v) for k, v in pooled.items()}
    ratios = SCORE_RATIOS + (("area_dice",) if areas else ())
    stats = {r: _defined_stats(table[r]) for r in ratios}
    out = {"n_images": n, "pooled": pooled, "mean": {r: stats[r][0] for r in ratios}, "median": {r: stats[r][1] for r in ratios},
           "defined": {r: stats[r][2] for r in ratios}}
    if groups is not None:
        out["n_groups"] = len(_group_index(groups, n)[0])
    if areas:
        e = np.asarray(table["area_error"], np.float64)
        bias = float(e.mean()) if n else float("nan")
        sd = float(e.std(ddof=1)) if n > 1 else float("nan")
        out["bland_altman"] = {"bias": bias, "sd": sd, "lower": bias - 1.96 * sd, "upper": bias + 1.96 * sd, "n": n}
    R = int(bootstrap)
    if R < 0:
        raise ValueError(f"bootstrap must be >= 0, got {bootstrap}")
    if R:
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
        from . import ops
        names, rows = bootstrap_rows(table, groups)
        U = rows.shape[0]
        if U == 0:
            raise ValueError("bootstrap: nothing to resample")
        ops.bootstrap_check_rows(int(np.abs(rows).max(initial=0)), U)
        dev = torch.device(device if device is not None else "cuda")
        sums = ops.bootstrap_sums(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), R, seed, check=False).cpu().numpy()
        st = bootstrap_statistics(names, sums, table.get("quantum"))
        intervals, dropped = {}, {}
        for k, v in st.items():
            ok = v[~np.isnan(v)]
            dropped[k] = int(v.size - ok.size)
            lo, hi = (np.quantile(ok, [alpha / 2.0, 1.0 - alpha / 2.0]) if ok.size else (float("nan"), float("nan")))
            intervals[k] = (float(lo), float(hi))
        out["bootstrap"] = {"replicates": R, "seed": int(seed), "alpha": float(alpha), "unit": "group" if groups is not None else "image", "units": U,
                            "intervals": intervals, "dropped": dropped}
    return out


def _lesion_measure(tm, geometry, connectivity):
    """uint8 [N,H,W] device mask -> (labels int32 device, counts int64 NumPy [N], measure int64 NumPy [N,cap,8]); one read-back sizes the table."""
    from . import ops
    if tuple(geometry.grid) != tuple(tm.shape[1:]):
        raise ValueError(f"lesion_sizes: the geometry is {tuple(geometry.grid)}, the masks {tuple(tm.shape[1:])}")
    labels, count = ops.label_components(tm, connectivity)
    count = count.cpu().numpy().astype(np.int64)
    cap = int(count.max()) if count.size else 0
    wq, xq, yq = geometry.tables(tm.device)
    return labels, count, ops.component_measure(labels, wq, xq, yq, cap).cpu().numpy()


def lesion_sizes_from_measure(count, measure, geometry):
    """``ops.component_measure``'s table -> per component, [N,cap] NumPy arrays in axis units: ``pixels``, ``area``, ``diameter`` = the
    equivalent diameter 2 sqrt(area / pi), ``centroid_x / centroid_y`` (area-weighted), ``x_min / x_max / y_min / y_max``; NaN (pixels 0) in
    the columns past an image's ``count``."""
    m = np.asarray(measure, np.int64)
    present = m[..., 0] > 0
    nan = lambda v: np.where(present, v, np.nan)
    area = geometry.area_of(m[..., 1])
    return {"count": np.asarray(count, np.int64), "pixels": m[..., 0], "area": nan(area), "diameter": nan(2.0 * np.sqrt(area / math.pi)),
            "centroid_x": nan(geometry.x_of(m[..., 2], m[..., 1])), "centroid_y": nan(geometry.y_of(m[..., 3], m[..., 1])),
            "x_min": nan(geometry.x_at(m[..., 4])), "x_max": nan(geometry.x_at(m[..., 5])),
            "y_min": nan(geometry.y_at(m[..., 6])), "y_max": nan(geometry.y_at(m[..., 7]))}


def lesion_sizes(mask, geometry, connectivity=8, device=None):
    """The size of every connected component of a stack of masks [N,H,W] in physical units, measured on the device
    (``ops.label_components`` + ``ops.component_measure``) -> ``lesion_sizes_from_measure``'s dict; component k of image n is column k-1,
    in ``scipy.ndimage.label``'s numbering."""
    dev = torch.device(device if device is not None else "cuda")
    _, count, measure = _lesion_measure(_mask_stack(mask, dev, "lesion_sizes"), geometry, connectivity)
    return lesion_sizes_from_measure(count, measure, geometry)
