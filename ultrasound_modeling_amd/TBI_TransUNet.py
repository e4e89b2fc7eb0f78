"""The surface of the reference's ``TBI_TransUNet.py`` (BASELINE configs[3]: ResNeSt encoder + ViT bottleneck + decoder,
512x512, batch 8, one GPU): an older, self-contained copy of the ResNest.py / Decoder.py / VisionTransformer.py model with

  * BatchNormalization (inference mode as driven) wherever the newer files use LayerNormalization
    (TBI_TransUNet.py:304 decoder bn1, :426 shortcut, :465 / :472 cardinal, :503 split attention),
  * ``conv_4 = residual_S(outchannel=256)`` (:368), so the 1x1 patch embedding maps 256 -> 512 (:110),
  * ``CategoricalCrossentropy(label_smoothing=0.1)`` with Keras' DEFAULT reduction - the mean over all B*H*W pixels (:546),
  * ``step(x, y, train=False) -> (loss, probabilities)`` (:571-588), clip-by-global-norm 1.0 and Adam, not jitted.

Everything runs on the same gfx950 kernels as the newer model (``VisionTransformer(..., transunet=True)``); the literal 16x5
token grid (:90,:547) is generalised to (H/16, W/16) as everywhere else.

The script's own ``main()`` path (:624-1010) is here too: ``label2vec``, ``Dataset``, its ``dataAug`` (``draw`` / ``dataAug_batch``),
``training``, ``test`` and ``main``.  Its ``dataAug`` (:835-875) is not ``DataAugs.dataAug``: it flips image and label left-right
when ``r % 2`` (:840-842) BEFORE anything else, runs ``imageReduc`` when ``r % 5 != 0`` (:844-845), clips ONE box when ``r % 3``
(:859-860), then shifts and adds noise on ``t % 2`` / ``t % 3`` (:869-873).  The whole batch is still one ``usseg_augment`` launch
(the flip is a per-sample remap of the source column).  Differences, all deliberate:
  * ``imageReduc(., r % 5)`` runs without its iteration count: the dilation never fires for any count >= 1 (:815, ``mask > 1`` on a
    0/1 mask), so every count only zeroes the image where the label is 0 - what the kernel does;
  * the Keras metric objects (:749-756) are ``metrics.SegMetrics`` counter buffers (``round=True``): one launch per batch and one
    read-back per epoch (train) or per test call; every call of ``test`` and every epoch of ``training`` starts from zero, and each
    epoch's numbers (loss included) are appended to the module's ``history`` as well as printed;
  * no TensorBoard summaries or image dumps (:748,:900-905,:958-962,:972-981), and the commented-out contrast / rotate blocks stay out;
  * the learning-rate reassignment at the end of every epoch (:927-932) changes attributes the plain-Adam optimiser never reads again
    (SURVEY.md appendix, quirk 6), so ``training`` keeps the fixed rate by default, like the reference.  ``schedule=True`` installs
    ``1e-3 * PiecewiseConstantDecay([10000, 20000, 40000, 60000, 80000], [1, .3, .1, .03, .01, .003])`` on the optimiser ONCE, before
    the first step, and ``1e-4 *`` the same schedule on the weight decay if the model runs AdamW; the optimiser evaluates it at its
    device step counter on every step (graph replays included);
  * the Gaussian of ``noisy`` comes from the device's counter-based generator seeded per sample (``DataAugs`` module docstring).
"""
from __future__ import annotations

import contextlib
import random
from typing import List, Optional

import torch

from . import DataAugs
from . import Dataset_2
from .MainNumpy import _labels, _raw_test_loss, average_setting, averaging, flush, install_schedule, paste_report
from .distill import distill_line
from .metrics import SegMetrics, dice_line
from .schedules import PiecewiseConstantDecay
from .VisionTransformer import VisionTransformer as _VisionTransformer, overlap_settings

input_size = (256, 80)      # :998-1004 (the model's defaults: 256x80, 10 channels)


class VisionTransformer(_VisionTransformer):
    """TBI_TransUNet.py:532-592.  Note the reference's argument order here: batch_size comes LAST (:533)."""

    def __init__(self, img_size=(256, 80), num_classes=3, learning_rate=1e-3, weight_decay=1e-4, batch_size=16, *,
                 in_channels: int = 10, device: Optional[str] = None, seed: Optional[int] = 0, adamw: bool = False,
                 loss: str = "cce", class_factor=None, focal_gamma=None, overlap=None,
                 alpha=None, beta=None, smooth=None, power=None, class_weight=None, ce_weight=None, ov_weight=None, boundary=None,
                 lovasz=None, average=None, topk=None, distill=None, teacher=None, accumulate=None):
        """``loss`` / ``class_factor`` / ``focal_gamma`` / ``overlap`` / ``boundary`` / ``lovasz`` / ``topk`` / ``distill`` + ``teacher``: as in the newer model (``VisionTransformer.VisionTransformer``), with this file's
        reduction - the mean over the B*H*W pixels of the batch (the overlap term of "dice" / "tversky" / "dice_ce" is a ratio of sums and has weight 1, and so
        has the Lovasz term of "lovasz" / "lovasz_ce"; "topk" is the mean over the selected pixels).  ``average``: the newer model's (EMA / SWA weight averaging)."""
        super().__init__(batch_size, img_size, num_classes, learning_rate, weight_decay, in_channels=in_channels, use_vit=True,
                         device=device, seed=seed, transunet=True, adamw=adamw, loss=loss, class_factor=class_factor, focal_gamma=focal_gamma,
                         overlap=overlap, alpha=alpha, beta=beta, smooth=smooth, power=power, class_weight=class_weight, ce_weight=ce_weight,
                         ov_weight=ov_weight, boundary=boundary, lovasz=lovasz, average=average, topk=topk, distill=distill, teacher=teacher, accumulate=accumulate)

    def step(self, x, y, train=False):
        """TBI_TransUNet.py:571-588 -> (loss, probabilities); ``train=True`` also clips and applies the gradients."""
        if train:
            return self.train_step(x, y)
        return super().step(x, y)


# ---------------------------------------------------------------------------------------------------- input pipeline (:624-875)
def label2vec(label: torch.Tensor) -> torch.Tensor:
    """:624-631 on the device: label [B,H,W] fp32 -> [B,H,W,3] fp32 (the 3-class map of Dataset_2.label2vec)."""
    return Dataset_2.label2vec(label, 3)


def draw(rng=random) -> dict:
    """The draws of one ``dataAug`` call (:835-875), in the script's order: r, t, then four for the clip box if ``r % 3``, then three
    for the shift if ``t % 2``.  ``reduc_t`` is the iteration count of :845, inert as executed (module docstring)."""
    r = rng.randint(0, 100000)
    t = rng.randint(0, 100000)
    p = {"flip": r % 2 == 1, "reduc": r % 5 != 0, "reduc_t": r % 5, "clips": [], "shift": None, "noise": bool(t % 3),
         "seed": r * 100003 + t}
    if r % 3:                                                                                                      # :859-860, ONE box
        p["clips"].append((rng.randint(0, 256), rng.randint(0, 80), rng.randint(20, 40), rng.randint(10, 20)))   # :780-783
    if t % 2:
        p["shift"] = (rng.randint(0, 30), rng.randint(0, 12), rng.randint(0, 1))                                  # :760-762
    return p


def dataAug_batch(x: torch.Tensor, y: torch.Tensor, params: Optional[List[dict]] = None, num_classes: int = 3,
                  noise: Optional[torch.Tensor] = None, rng=random, want_f32: bool = False):
    """``DataAugs.dataAug_batch`` driven by this script's ``draw``: the whole batch (flip included) in one ``usseg_augment`` launch."""
    if params is None:
        params = [draw(rng) for _ in range(x.shape[0])]
    return DataAugs.dataAug_batch(x, y, params=params, num_classes=num_classes, noise=noise, want_f32=want_f32)


def dataAug(image: torch.Tensor, label: torch.Tensor):
    """Single-sample form with the script's signature (:835): image [H,W,C], label [H,W] -> (image fp32, label)."""
    _, _, xf, ya = dataAug_batch(image[None], label[None].float(), want_f32=True)
    return xf[0], ya[0]


class Dataset(Dataset_2.Dataset):
    """:634-745: ``Dataset_2.Dataset``'s layout and bookkeeping (resident in HBM, device tensors out) with 3 classes and this script's
    ``dataAug`` in ``next_train``; ``next_test`` does not augment."""
    draw = staticmethod(draw)

    def __init__(self, train_path=None, val_path=None, device="cuda", train_data=None, val_data=None, warp=None, warp_seed=0,
                 paste=None, paste_seed=0):
        super().__init__(train_path, val_path, num_classes=3, device=device, train_data=train_data, val_data=val_data, warp=warp, warp_seed=warp_seed,
                         paste=paste, paste_seed=paste_seed)
        self.num_class = 3                                                                         # :682


# ---------------------------------------------------------------------------------------------------- drivers (:877-1010)
history = []     # one dict per training epoch (``phase`` "train") and per test() call (``phase`` "test")


def reference_schedule() -> PiecewiseConstantDecay:
    """:927-928."""
    return PiecewiseConstantDecay([10000, 20000, 40000, 60000, 80000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])


def training(neuralnet, dataset, epochs, batch_size, *, schedule=False):
    """:877-935: epochs from 0; train-set Recall / Precision / MeanIoU of every step; ``test`` when ``epoch % 5 == 0``.  ``schedule``:
    see the module docstring.  -> the number of steps taken."""
    print("\nTraining to %d epochs (%d of minibatch size)" % (epochs, batch_size))
    if schedule:
        install_schedule(neuralnet, reference_schedule(), lr_scale=1e-3, wd_scale=1e-4)
    tr_metrics = SegMetrics(3, round=True, device=neuralnet.device)        # tr_recall / tr_precision / tr_mio (:754-756)
    iteration = 0
    prev_loss = 0
    for epoch in range(epochs):
        while True:
            x_tr, y_tr, terminator = dataset.next_train(batch_size)                                  # :888
            loss, class_score = neuralnet.step(x=x_tr, y=y_tr, train=True)                           # :890
            iteration += 1
            tr_metrics.update_state(_labels(y_tr, class_score), class_score)                         # :893-898, read back per epoch
            print('.', end='')
            if (iteration + 1) % 100 == 0:
                print()
            if terminator:
                break
        flush(neuralnet)            # accumulate=N: a short last group still takes its optimiser step, before validation and saving
        print()
        loss = float(loss)          # the epoch's last step (:892 reduce_sum of a scalar); after a graph replay the static buffer
        m = tr_metrics.result()
        print("Epoch [%d / %d] (%d iteration)  Loss:%.5f, Recall:%.5f, Precision:%.5f, IoU:%.5f"
              % (epoch, epochs, iteration, loss, m["recall"], m["precision"], m["mean_iou"]))
        history.append(dict(m, phase="train", epoch=epoch, iteration=iteration, loss=loss))
        paste_report(dataset)
        tr_metrics.reset_states()                                                                    # :917-919
        if prev_loss == loss:
            print("Model is throwing a fit")
            print(class_score)
        prev_loss = loss
        if epoch % 5 == 0:
            test(neuralnet, dataset, epoch)
        # :927-932 (the rate reassignment): installed before the first step with schedule=True, see the module docstring
    return iteration


def test(neuralnet, dataset, epoch):
    """:938-994 -> F1 of the test set (batches of 16, labels and probabilities rounded); loss = the sum of the batch losses / num_te
    (:968).  Its dict (``phase`` "test") is appended to ``history``."""
    print("\nTest...")
    m = SegMetrics(3, round=True, device=neuralnet.device)             # precision / recall / pre_c2 / re_c2 / mio (:749-753)
    averaged = averaging(neuralnet)   # built with average=: the averaged model is tested, the raw loss reported too
    extra = {"raw_loss": _raw_test_loss(neuralnet, dataset) / dataset.num_te} if averaged else {}
    total_loss = None
    with (neuralnet.averaged_weights() if averaged else contextlib.nullcontext()):
        while True:
            x_te, y_te, terminator = dataset.next_test(16)                                           # :946
            loss, class_score = neuralnet.step(x=x_te, y=y_te, train=False)                          # :947
            total_loss = loss.detach().reshape(()).clone() if total_loss is None else total_loss.add_(loss.reshape(()))   # :956, on the device
            m.update_state(_labels(y_te, class_score), class_score)                                  # :949-956
            if terminator:
                break
    total_loss = float(total_loss) / dataset.num_te                                                  # :968
    r = m.result()
    print("loss = {}".format(total_loss))
    if averaged:
        print("loss (raw weights) = {}".format(extra["raw_loss"]))
    print("IoU = {}".format(r["mean_iou"]))
    print("f1 = {}".format(r["f1"]))
    print("precision = {}".format(r["precision"]))
    print("recall = {}".format(r["recall"]))
    dice = dice_line(neuralnet, m)
    if dice is not None:                                        # only with loss="dice" / "tversky" / "dice_ce"
        print("dice per class = {}".format(dice))
    terms = distill_line(neuralnet)
    if terms is not None:                                       # only with loss="distill": the last validation batch's two terms
        print("distill terms: {}".format(terms))
    history.append(dict(r, phase="test", epoch=epoch, loss=total_loss, **extra))
    return r["f1"]


def main(train_path, val_path, save_path=None, epochs=51, batch_size=16, *, loss="cce", overlap=None, boundary=None, lovasz=None, average=None,
         warp=None, warp_seed=0, topk=None, teacher=None, distill=None, accumulate=None, paste=None, paste_seed=0):
    """:997-1010 with the paths as arguments: 256x80x10 input, batch 16, 51 epochs, then a save if ``save_path`` is given.
    ``loss``: the model's ``loss=`` ("cce", "my_loss_cat", "focal", "dice", "tversky", "dice_ce"); ``overlap``: the settings of the last three,
    which also add a per-class Dice line to the test report; ``boundary``: the boundary term on top of one of those three; "lovasz" / "lovasz_ce" with their
    settings in ``lovasz`` (the Lovasz-softmax loss; the Dice line too).  ``average`` (a dict, or ``ema:DECAY[:dynamic]`` / ``swa:START:PERIOD``):
    EMA / SWA weight averaging - ``test`` reports the averaged model and the save also writes ``<save_path>.avg`` (``save_averaged``).
    ``warp`` (a ``warp.warp_config`` dict or ``parse_warp`` string; default off): elastic / affine warp of every training batch ahead of ``dataAug``.
    "topk" / "dice_topk" with their settings in ``topk`` (the top-k cross-entropy; the Dice line too).
    "distill" with ``teacher`` (a model, an ``Ensemble``, or checkpoint paths of this file's model - a list or a comma-separated string; several
    make an ensemble) and its settings in ``distill``: knowledge distillation; the test report adds the two terms of the last validation batch.
    ``accumulate`` (an integer N >= 1; None: 1): every ``batch_size`` batch is a micro-batch and N of them make one optimiser step (DESIGN.md section
    4g-3); ``training`` flushes a short last group at the end of every epoch, before ``test`` and the save.
    ``paste`` (a ``paste.paste_config`` dict or ``parse_paste`` string; default off): lesions of the training set are pasted into every training batch
    ahead of the warp, its draws from ``random.Random(paste_seed)``; ``training`` prints one line per epoch: lesions placed of drawn."""
    dataset = Dataset(train_path, val_path, warp=warp, warp_seed=warp_seed, paste=paste, paste_seed=paste_seed)
    kw = {} if topk is None else {"topk": topk}
    if teacher is not None or distill is not None:
        if isinstance(teacher, (str, list, tuple)):
            from .distill import load_teacher
            teacher = load_teacher(teacher, input_size, 10, "cuda", transunet=True)
        kw.update(teacher=teacher, distill=distill)
    neuralnet = VisionTransformer(img_size=input_size, num_classes=3, learning_rate=1e-3, batch_size=batch_size, loss=loss, overlap=overlap_settings(loss, overlap),
                                  boundary=boundary, lovasz=lovasz, average=average_setting(average), accumulate=accumulate, **kw)
    print(len(neuralnet.visionModel.layers))
    training(neuralnet=neuralnet, dataset=dataset, epochs=epochs, batch_size=batch_size)
    if save_path is not None:
        neuralnet.visionModel.save(save_path)
        if average is not None:
            neuralnet.save_averaged(save_path + ".avg")
    return neuralnet
