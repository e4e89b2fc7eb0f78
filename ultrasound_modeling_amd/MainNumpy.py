"""The reference's single-GPU training / test driver (``MainNumpy.py:14-147``) with its validation metrics counted on the device.

``Process(batch_size, num_classes).training(neuralnet, dataset, epochs)`` and ``.test(neuralnet, dataset, epoch)`` drive any
model with ``train_step(x, y) -> (loss, probs)`` and ``step(x, y) -> (loss, probs)`` (VisionTransformer, TBI_TransUNet) over a
``Dataset_2.Dataset``.  Differences, all deliberate:
  * the eight Keras metric objects (:20-27) are two ``metrics.SegMetrics`` counter buffers: one launch per batch, stream-ordered
    behind the step that produced the probabilities (also behind a replayed HIP graph, whose ``probs`` is the static buffer), and
    ONE read-back per epoch instead of a host read of five metric objects;
  * every metric is reset after the epoch that reported it, and each epoch's numbers (loss included) are appended to
    ``self.history`` as well as printed;
  * no TensorBoard summaries or image dumps (:16-17,54-60,108-113,124-133);
  * the learning-rate "schedule" (:83-88) is off by default: the reference reassigns ``neuralnet.learning_rate`` / ``weight_decay``
    at every epoch's end, plain attributes its optimiser never reads again, so it trains at the fixed
    rate the model was built with, and so does this driver.  ``Process(..., schedule=True)`` applies what :83-88 meant instead: the
    schedule ``PiecewiseConstantDecay([2000, 4000, 8000, 10000, 15000], [1, .3, .1, .03, .01, .003])`` is installed ONCE, before the
    first step, as ``1e-2 * schedule`` on the learning rate and - if the model runs AdamW (``adamw=True``) - ``1e-4 * schedule`` on
    the weight decay.  The optimiser evaluates it at its device step counter on every step (graph replays included), where the
    reference would have evaluated it at epoch ends only.
"""
from __future__ import annotations

import contextlib

import torch

from .distill import distill_line
from .metrics import SegMetrics, dice_line
from .schedules import PiecewiseConstantDecay

input_size = (256, 80)      # :12


class Process(object):
    def __init__(self, batch_size=16, num_classes=3, device=None, schedule=False, surface=None, calibration=None, sweep=None):
        self.batch_size = batch_size
        # threshold sweep of ``test`` (default off): {"bins": 1024, "cls": -1} (metrics.SweepCounts' arguments)
        self.sweep = None
        if sweep is not None:
            from .metrics import SweepCounts
            if not isinstance(sweep, dict) or set(sweep) - {"bins", "cls"}:
                raise ValueError(f"sweep takes a dict with 'bins' and 'cls', got {sweep!r}")
            self.sweep = SweepCounts(sweep.get("bins", 1024), sweep.get("cls", -1), device=device if device is not None else "cuda")
        # reliability counters of ``test`` (default off): {"bins": 15, "cls": -1} (metrics.CalibrationBins' arguments)
        self.calibration = None
        if calibration is not None:
            from .metrics import CalibrationBins
            if not isinstance(calibration, dict) or set(calibration) - {"bins", "cls"}:
                raise ValueError(f"calibration takes a dict with 'bins' and 'cls', got {calibration!r}")
            self.calibration = CalibrationBins(calibration.get("bins", 15), calibration.get("cls", -1), device=device if device is not None else "cuda")
        # surface scores of the last class in ``test`` (default off): {"percentiles": [...], "tolerances": [...]} (metrics.surface_distances' arguments)
        self.surface = None if surface is None else surface_settings(surface)
        self.schedule = schedule            # apply the :83-88 learning-rate / weight-decay schedule (module docstring)
        self.num_classes = num_classes
        self.input_shape = [input_size[0], input_size[1], 10]                                    # :19
        dev = device if device is not None else "cuda"
        self.metrics = SegMetrics(num_classes, round=True, device=dev)        # precision / recall / pre_c2 / re_c2 / mio (:20-24)
        self.tr_metrics = SegMetrics(num_classes, round=True, device=dev)     # tr_recall / tr_precision / tr_mio (:25-27)
        self.test_iter = 0
        self.history = []

    def training(self, neuralnet, dataset, epochs, *, boundary_ramp=None):
        """MainNumpy.py:31-88 -> None; one dict per epoch in ``self.history`` (``phase`` "train").  ``boundary_ramp`` (default off): added to the model's boundary
        weight after each epoch - Kervadec et al.'s rebalancing; the weight is a device float, so a captured graph follows it."""
        print("\nTraining to %d epochs (%d of minibatch size)" % (epochs, self.batch_size))
        iteration = 0
        prev_loss = 0
        if self.schedule:
            install_schedule(neuralnet)
        for epoch in range(1, epochs + 1):
            while True:
                x_tr, y_tr, terminator = dataset.next_train(self.batch_size)                     # :43
                loss, class_score = neuralnet.train_step(x=x_tr, y=y_tr)                         # :45
                iteration += 1
                self.tr_metrics.update_state(_labels(y_tr, class_score), class_score)            # :49-53, read back once per epoch
                print('.', end='')
                if (iteration + 1) % 100 == 0:
                    print()
                if terminator:
                    break
            flush(neuralnet)        # accumulate=N: a short last group still takes its optimiser step, before validation and saving
            print()
            loss = float(loss)      # the epoch's last step (:47,70: reduce_sum of a scalar); after a graph replay the static buffer
            m = self.tr_metrics.result()
            print("Epoch [%d / %d] (%d iteration)  Loss:%.5f, Recall:%.5f, Precision:%.5f, IoU:%.5f"
                  % (epoch, epochs, iteration, loss, m["recall"], m["precision"], m["mean_iou"]))
            self.history.append(dict(m, phase="train", epoch=epoch, iteration=iteration, loss=loss))
            self.tr_metrics.reset_states()                                                       # :73-75
            paste_report(dataset)
            if prev_loss == loss:
                print("Model is throwing a fit")
                print(class_score)
            prev_loss = loss
            if boundary_ramp is not None:
                neuralnet.set_boundary_weight(neuralnet.boundary_weight + float(boundary_ramp))
            if epoch % 5 == 0:
                self.test(neuralnet, dataset, epoch)
            # :83-88 (the learning-rate "schedule"): installed before the first step with schedule=True, see the module docstring

    def test(self, neuralnet, dataset, epoch):
        """MainNumpy.py:90-147 -> F1 of the epoch's test set; its dict (``phase`` "test") is appended to ``self.history``.  A model built with
        ``average=`` is validated under ``averaged_weights()`` - loss, counters, Dice line and the optional surface / calibration / sweep
        scores are the averaged model's - and the report adds the loss of the raw weights (``raw_loss`` in the history)."""
        print("\nTest...")
        total_loss = None
        stats = []                                              # per batch: usseg_surface_stats' four tensors, left on the device
        averaged = averaging(neuralnet)
        raw_loss = _raw_test_loss(neuralnet, dataset) if averaged else None      # the weights as they stand, for comparison
        with (neuralnet.averaged_weights() if averaged else contextlib.nullcontext()):       # everything scored below: the averaged model
            while True:
                x_te, y_te, terminator = dataset.next_test(16)                                       # :97
                loss, class_score = neuralnet.step(x=x_te, y=y_te)                                   # :98
                total_loss = loss.detach().reshape(()).clone() if total_loss is None else total_loss.add_(loss.reshape(()))   # :107, on the device
                labels = _labels(y_te, class_score)
                self.metrics.update_state(labels, class_score)                                       # :100-106
                if self.surface is not None:
                    stats.append(_surface_batch(labels, class_score, self.num_classes, self.surface))
                if self.calibration is not None:
                    self.calibration.update(class_score, labels)
                if self.sweep is not None:
                    self.sweep.update(class_score, labels)
                if terminator:
                    break
                self.test_iter += 1
        total_loss = float(total_loss)
        m = self.metrics.result()
        print("loss = {}".format(total_loss))
        if averaged:
            print("loss (raw weights) = {}".format(raw_loss))
        print("IoU = {}".format(m["mean_iou"]))
        print("f1 = {}".format(m["f1"]))
        print("precision = {}".format(m["precision"]))
        print("recall = {}".format(m["recall"]))
        dice = dice_line(neuralnet, self.metrics)
        if dice is not None:                                    # only with loss="dice" / "tversky" / "dice_ce"
            print("dice per class = {}".format(dice))
        terms = distill_line(neuralnet)
        if terms is not None:                                   # only with loss="distill": the last validation batch's two terms
            print("distill terms: {}".format(terms))
        extra = {"raw_loss": raw_loss} if averaged else {}
        if self.surface is not None:
            extra = dict(extra, **surface_summary(stats, self.surface))       # ONE read-back of the epoch's integers
            print(surface_line(extra, self.surface))
        if self.calibration is not None:
            from .metrics import calibration_line
            cal = self.calibration.result()                    # ONE read-back of the epoch's counters
            print(calibration_line(cal))
            extra = dict(extra, ece=cal["ece"], mce=cal["mce"], brier=cal["brier"])
            self.calibration.reset()
        if self.sweep is not None:
            from .metrics import sweep_line
            sw = self.sweep.result()                           # ONE read-back of the epoch's counters
            print(sweep_line(sw))
            extra = dict(extra, auc=sw["auc"], average_precision=sw["average_precision"], best_dice=sw["best_dice"][2],
                         best_dice_threshold=sw["best_dice"][1])
            self.sweep.reset()
        self.history.append(dict(m, phase="test", epoch=epoch, loss=total_loss, **extra))
        self.metrics.reset_states()                                                              # :142-146
        return m["f1"]


def main(train_path, val_path, save_path=None, epochs=50, batch_size=32, num_classes=3, *, loss="cce", overlap=None, boundary=None, lovasz=None,
         average=None, warp=None, warp_seed=0, topk=None, teacher=None, distill=None, accumulate=None, paste=None, paste_seed=0):
    """MainNumpy.py:150-177 with the paths as arguments: ``VisionTransformer(32, img_size=(256, 80))`` over a ``Dataset_2.Dataset``,
    50 epochs, then a save if ``save_path`` is given.  ``loss``: the model's ``loss=`` ("cce", "my_loss_cat", "focal", "dice", "tversky",
    "dice_ce"); ``overlap``: the settings of the last three (``VisionTransformer(overlap=...)``), which also add a per-class Dice line to the test report;
    ``boundary``: the boundary term on top of one of those three (``VisionTransformer(boundary=...)``); "lovasz" / "lovasz_ce" with their settings in
    ``lovasz`` (``VisionTransformer(lovasz=...)``: the Lovasz-softmax loss; the Dice line too).  ``average`` (a dict, or the string
    ``ema:DECAY[:dynamic]`` / ``swa:START:PERIOD``): EMA / SWA weight averaging - the tests report the averaged model, and the save also writes
    ``<save_path>.avg``, a plain checkpoint of the averaged weights (``save_averaged``).  ``warp`` (a ``warp.warp_config`` dict or ``parse_warp``
    string; default off): elastic / affine warp of every training batch ahead of ``dataAug``, its draws from ``random.Random(warp_seed)``.
    "topk" / "dice_topk" with their settings in ``topk`` (``VisionTransformer(topk=...)``: the top-k cross-entropy; the Dice line too).
    "distill" with ``teacher`` (a model, an ``Ensemble``, or checkpoint paths - a list or a comma-separated string; several make an ensemble) and
    its settings in ``distill`` (``VisionTransformer(distill=...)``): knowledge distillation; the test report adds the hard and soft terms of
    the last validation batch.  ``accumulate`` (an integer N >= 1; None: 1): ``VisionTransformer(accumulate=N)`` - every ``batch_size`` batch is a
    micro-batch and N of them make one optimiser step; a short last group of an epoch is flushed before validation and saving, and the epoch
    loss stays the last micro-batch's.  ``paste`` (a ``paste.paste_config`` dict or ``parse_paste`` string; default off): lesions of the training set
    are pasted into every training batch ahead of the warp, its draws from ``random.Random(paste_seed)``; ``training`` then
    prints one line per epoch: lesions placed of lesions drawn, and the pixels pasted."""
    from .Dataset_2 import Dataset
    from .VisionTransformer import VisionTransformer, overlap_settings
    dataset = Dataset(train_path, val_path, num_classes, warp=warp, warp_seed=warp_seed, paste=paste, paste_seed=paste_seed)
    kw = {} if topk is None else {"topk": topk}
    if teacher is not None or distill is not None:
        if isinstance(teacher, (str, list, tuple)):
            from .distill import load_teacher
            teacher = load_teacher(teacher, input_size, 10, "cuda", num_classes=num_classes)
        kw.update(teacher=teacher, distill=distill)
    neuralnet = VisionTransformer(batch_size, img_size=input_size, num_classes=num_classes, loss=loss, overlap=overlap_settings(loss, overlap),
                                  boundary=boundary, lovasz=lovasz, average=average_setting(average), accumulate=accumulate, **kw)
    print(len(neuralnet.visionModel.layers))
    process = Process(batch_size=batch_size, num_classes=num_classes)
    process.training(neuralnet=neuralnet, dataset=dataset, epochs=epochs)
    if save_path is not None:
        neuralnet.visionModel.save(save_path)
        if average is not None:
            neuralnet.save_averaged(save_path + ".avg")
    return neuralnet, process


def paste_report(dataset, show=print):
    """With ``paste=``: the epoch's line - lesions placed out of lesions drawn, pixels pasted - from ONE read-back of the dataset's device counters
    -> (placed, drawn, pixels); None, and nothing printed or read, without."""
    fn = getattr(dataset, "paste_report", None)
    rep = fn() if fn is not None else None
    if rep is not None:
        from .paste import paste_line
        show(paste_line(*rep))
    return rep


def flush(neuralnet):
    """``flush_step()`` of a model that has it (``step.TrainStepDriver``; nothing pending: nothing happens): the end of an epoch's training loop."""
    fn = getattr(neuralnet, "flush_step", None)
    if fn is not None:
        fn()


def averaging(neuralnet) -> bool:
    """Whether the model's optimiser keeps averaged weights (``flat.AdamClip(average=...)``)."""
    return getattr(getattr(neuralnet, "optimizer", None), "avg", None) is not None


def average_setting(average):
    """``average`` of the drivers' ``main``: None, the ``AdamClip(average=...)`` dict, or the command-line string."""
    if isinstance(average, str):
        from .flat import parse_average
        return parse_average(average)
    return average


def _raw_test_loss(neuralnet, dataset) -> float:
    """One more pass over the test set (batches of 16) for the summed loss alone."""
    total = None
    while True:
        x_te, y_te, terminator = dataset.next_test(16)
        loss, _ = neuralnet.step(x=x_te, y=y_te)
        total = loss.detach().reshape(()).clone() if total is None else total.add_(loss.reshape(()))
        if terminator:
            return float(total)


def reference_schedule() -> PiecewiseConstantDecay:
    """MainNumpy.py:83-84."""
    return PiecewiseConstantDecay([2000, 4000, 8000, 10000, 15000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])


def install_schedule(neuralnet, schedule=None, lr_scale=1e-2, wd_scale=1e-4):
    """MainNumpy.py:86-87 on the model's optimiser: lr = 1e-2 * schedule, and wd = 1e-4 * schedule if the model runs AdamW.
    ``schedule`` (default ``reference_schedule()``) and the two scales let the other drivers install their own (TBI_TransUNet.py:927-932)."""
    schedule = reference_schedule() if schedule is None else schedule
    opt = neuralnet.optimizer
    neuralnet.learning_rate = lr_scale * schedule
    opt.set_learning_rate(neuralnet.learning_rate)
    if opt.weight_decay is not None:
        neuralnet.weight_decay = wd_scale * schedule
        opt.set_weight_decay(neuralnet.weight_decay)


def surface_settings(surface):
    """``Process(surface=...)`` -> {"percentiles": [...], "tolerances": [...], "tol2": [...]}; ValueError for anything ``metrics.surface_distances`` refuses."""
    from .metrics import _percentile_list, _tolerance_list
    if not isinstance(surface, dict) or set(surface) - {"percentiles", "tolerances"}:
        raise ValueError(f"surface: a dict with 'percentiles' and / or 'tolerances', got {surface!r}")
    ts, t2 = _tolerance_list(surface.get("tolerances"))
    return {"percentiles": _percentile_list(surface.get("percentiles")), "tolerances": ts, "tol2": t2}


def _surface_batch(labels, probs, num_classes, cfg):
    """One validation batch's ``usseg_surface_stats`` of the last class: the prediction ``argmax == num_classes - 1`` against the label plane ``> 0.5``.
    Stream-ordered behind the step; nothing is read back."""
    from . import ops
    c = num_classes - 1
    pred = (probs[..., :num_classes].argmax(-1) == c).to(torch.uint8).contiguous()
    true = (labels[..., c] > 0.5).to(torch.uint8).contiguous()
    return ops.surface_stats(pred, true, cfg["percentiles"], cfg["tol2"])


def surface_summary(stats, cfg):
    """The epoch's per-batch device results -> history keys: the means over the scored images of each percentile (pooled and directed) and of the surface
    Dice at each tolerance, ``surface_scored`` (images where both surfaces exist: their HD is not NaN), ``surface_nsd_scored`` (images with at least one
    surface) and ``surface_images``."""
    import numpy as np
    from .metrics import surface_scores_from_stats
    parts = [torch.cat([s[i] for s in stats]).cpu() for i in range(4)]
    s = surface_scores_from_stats(*parts, cfg["percentiles"], cfg["tolerances"])
    ok, ok_nsd = ~np.isnan(s["hd"]), (s["n_a"] + s["n_b"]) > 0

    def mean(col, keep):
        v = [float(x) for x in col[keep]]
        return sum(v) / len(v) if v else float("nan")
    return {"surface_hd_pct": [mean(s["hd_pct"][:, p], ok) for p in range(len(cfg["percentiles"]))],
            "surface_hd_pct_directed": [mean(s["hd_pct_directed"][:, p], ok) for p in range(len(cfg["percentiles"]))],
            "surface_nsd": [mean(s["nsd"][:, t], ok_nsd) for t in range(len(cfg["tolerances"]))],
            "surface_scored": int(ok.sum()), "surface_nsd_scored": int(ok_nsd.sum()), "surface_images": int(ok.shape[0])}


def surface_line(summary, cfg):
    """The report line after the Dice line."""
    from .TBIEvaluator import _column_number
    parts = []
    for p, q in enumerate(cfg["percentiles"]):
        parts.append("hd{} = {}, hd{}_directed = {}".format(_column_number(q), summary["surface_hd_pct"][p], _column_number(q), summary["surface_hd_pct_directed"][p]))
    for t, tau in enumerate(cfg["tolerances"]):
        parts.append("nsd{} = {}".format(_column_number(tau), summary["surface_nsd"][t]))
    return "surface (mean over scored images): {} ({} of {} images have both surfaces, {} at least one)".format(
        ", ".join(parts), summary["surface_scored"], summary["surface_images"], summary["surface_nsd_scored"])


def _labels(y, probs):
    """The labels the step consumed, as the fp32 contiguous device tensor the counting kernel reads (the model's own _prep_y)."""
    return torch.as_tensor(y).to(device=probs.device, dtype=torch.float32).contiguous()
