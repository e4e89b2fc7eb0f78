"""Single-node data parallelism with the semantics of the reference's ``MainParallel.py`` (MirroredStrategy).

Reference behaviour being mirrored (MainParallel.py:16,117-146,209-210):
  * variables are created once and mirrored on every GPU (:209-210)  -> rank 0's flat parameter buffer is broadcast;
  * each global batch is split into N contiguous per-replica slices (:127-128) -> ``shard_batch``;
  * every replica runs ``train_step`` on its slice with the loss divided by the GLOBAL batch size
    (VisionTransformer.py:227), clips ITS OWN gradients by global norm (:244), and ``apply_gradients`` then
    all-reduces them with SUM before the identical Adam update on every replica (:245 under :130);
  * scalar metrics are SUM-reduced (:131-134) and evaluation outputs gathered (:160,:163).
MI355X design: one process per GPU (torchrun), ONE RCCL all-reduce over the flat fp32 gradient buffer per step
(25 MB for the conv-only Arch B): on the fully connected xGMI node a single large collective uses all 7 links.
BatchNorm statistics are NOT synchronised (the reference uses plain BatchNormalization, ResNest.py:19).
Validation metrics (:86-114,148-176): instead of gathering every replica's probabilities and labels (``test_step`` still does,
as the reference), a replica counts its own slice with ``metrics.SegMetrics.update_state`` and calls ``SegMetrics.reduce()`` (a SUM
all-reduce of 23 int64 counters, exact) before ``result()``: the numbers of one process on the concatenated batch.

The epoch driver (``Process.training`` / ``test`` / ``mirrored_train_step`` / ``mirrored_test_step``, ``main`` and the command line,
MainParallel.py:24-176,201-220) runs any model with ``train_step`` / ``step`` / ``empty_step`` (``VisionTransformer``) over a
``Dataset.Dataset``, one process per replica:
    python -m torch.distributed.run --nproc_per_node N -m ultrasound_modeling_amd.MainParallel TRAIN VAL [--save P] [--epochs N]
        [--batch-size B] [--no-vit] [--loss {cce,my_loss_cat,focal,dice,tversky,dice_ce}]
(world size 1 runs without the launcher).  As the reference executes: epochs count from 0; ``test`` runs after EVERY epoch (:72); the
test loss is the plain sum over the test batches (:89 is commented out); test batches are ``batch_size`` images (:155) split like the
training batches; each replica's loss is divided by the GLOBAL batch (``VisionTransformer.batch_size``, a short last batch included,
``compute_average_loss(global_batch_size=...)``); the printed training loss is the last step's SUM-reduced loss (:131,146); "Model is
throwing a fit" on an equal loss (:69-70); BatchNorm statistics stay per replica; only rank 0 saves.  The loss and the counters stay on
the device: ONE loss all-reduce and ONE ``SegMetrics.reduce()`` per epoch and per ``test`` call, no gather and no per-step host read.
A replica whose share of a short last batch is empty still joins the step (``TrainStepDriver.empty_step``: zero gradient, the same
exchange and update) and adds 0 to the loss and nothing to the counters.  Full local batches replay the captured two-graph step
(``capture_graph`` on the first one; ``Process(capture_graph=False)`` keeps every step eager); any other local batch runs eagerly.
Deliberate deviations:
  * the reference driver cannot run as committed: it unpacks five values from a ``train_step`` that returns two (:130, SURVEY.md:143)
    and its metric attributes are the int 0 (:30-37).  The training Recall / Precision / IoU are counted from each step's
    probabilities, as ``MainNumpy`` does (``SegMetrics(3, round=True)``, reset after every epoch);
  * the rate reassignment after every epoch (:74-79) sets attributes the plain Adam never reads again,
    so the driver trains at the fixed rate by default.  ``Process(schedule=True)`` installs ``1e-3 * PiecewiseConstantDecay([10000,
    20000, 40000, 60000, 80000], [1, .3, .1, .03, .01, .003])`` ONCE, before the first step (``MainNumpy.install_schedule``; ``1e-4 *``
    the same on the weight decay under AdamW), evaluated by the optimiser at its device step counter; the ``learning_rate < 1e-5`` stop
    (:49) reads ``optimizer.current_learning_rate()`` once per epoch;
  * no TensorBoard scalars or image summaries (:26-27,93-102,136-139,171-174).
"""
from __future__ import annotations

import argparse
import contextlib
import os
import random
from typing import Optional, Tuple

import torch
import torch.distributed as dist
from . import knobs
from .MainNumpy import averaging, flush
from .distill import distill_line
from .metrics import dice_line


def init_distributed(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """Initialise torch.distributed from the torchrun environment. -> (rank, world_size, local_rank)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            # USSEG_DIST_BACKEND=gloo: rehearsal of the multi-process path on a box with fewer GPUs than ranks (the ranks then
            # share a device and the exchange goes through host memory - correctness only, never a measurement)
            backend = knobs.get("USSEG_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")   # "nccl" is RCCL on ROCm
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def shard_batch(x, y, rank: int, world: int):
    """The contiguous per-replica slice of a global batch (experimental_distribute_dataset, MainParallel.py:128)."""
    B = x.shape[0]
    assert B % world == 0, "global batch must divide evenly over the replicas"
    n = B // world
    return x[rank * n:(rank + 1) * n], y[rank * n:(rank + 1) * n]


class GradSync:
    """The gradient exchange of ``apply_gradients`` under MirroredStrategy: SUM all-reduce of the flat fp32 gradient buffer.

    ``nchunks == 1``: ONE collective over the whole buffer (the update then replays as a second HIP graph).
    ``nchunks > 1``: the buffer is exchanged as ``nchunks`` contiguous pieces issued back to back on RCCL's stream; the step
    driver (step.TrainStepDriver._sync_and_update) waits for piece k ON THE COMPUTE STREAM (an event wait, the host does not
    block) and runs the Adam kernel of that range while piece k+1 is still on the wire.  Exact: the per-replica clip already
    happened (VisionTransformer.py:244 precedes :245), and both the SUM and Adam are elementwise over the flat buffer.
    What can NOT be overlapped exactly is the exchange with the backward pass: the reference reduces c_r*g_r where the
    per-replica clip factor c_r = min(1, 1/||g_r||) needs the whole local gradient first."""

    def __init__(self, group=None, nchunks: int = 1, align: int = 1 << 16):
        self.group, self.nchunks, self.align = group, max(1, int(nchunks)), align
        if self.nchunks == 1:
            self.chunks = None               # the driver checks this attribute

    def __call__(self, flat_grad: torch.Tensor):
        dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=self.group)

    def chunks(self, flat_grad: torch.Tensor):
        from .step import even_chunks
        ranges = even_chunks(flat_grad.numel(), self.nchunks, self.align)
        works = [dist.all_reduce(flat_grad[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True) for lo, hi in ranges]
        for (lo, hi), w in zip(ranges, works):
            yield lo, hi, w.wait


class MirroredTrainer:
    """Wraps a model that has ``flat`` (FlatParams), ``grad_sync`` and ``train_step`` (VisionTransformer / Arch A).

    ``chunks``: pieces the gradient exchange is pipelined in (None / 1 = ONE collective and a graph-replayed update - the default;
    k > 1 = k pieces with the Adam kernel of piece i under the wire time of piece i+1, see GradSync).  Measured on one GPU
    (RCCL group of one rank, so no wire time to hide): the chunked form's eagerly launched update costs Arch A +0.2 ms per step
    (7.88 vs 7.68 ms) against at most 0.12 ms of Adam time it could hide behind a 103 MB all-reduce - so it stays opt-in
    (``USSEG_DP_CHUNKS`` / ``bench.py --dp-chunks``) until it can be measured on an 8-GPU node."""

    def __init__(self, net, group=None, force: bool = False, chunks: Optional[int] = None):
        self.net, self.group = net, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if self.world > 1 or (force and dist.is_initialized()):
            dist.broadcast(net.flat.flat, src=0, group=group)          # mirrored variables (:209-210)
            for m in net.modules():
                for b in m._buffers.values():
                    if b is not None:
                        dist.broadcast(b, src=0, group=group)
            if hasattr(net, "repack"):
                net.repack()
            if chunks is None:
                chunks = knobs.get("USSEG_DP_CHUNKS") or 1
            net.grad_sync = GradSync(group, chunks)

    def train_step(self, x_local, y_local):
        """One mirrored step on this replica's slice -> (global loss, local probs) (MainParallel.py:130-131)."""
        loss, probs = self.net.train_step(x_local, y_local)
        if self.world > 1:
            loss = loss.clone()
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=self.group)
        return loss, probs

    def test_step(self, x_local, y_local):
        """mirrored_test_step (MainParallel.py:148-176): SUM-reduced loss (:159), the probabilities of all replicas gathered along
        the batch axis (:160) and the labels likewise (:163) -> (loss, probs [B_global,...], y [B_global,...])."""
        loss, probs = getattr(self.net, "eval_step", self.net.step)(x_local, y_local)
        y = y_local
        if self.world > 1:
            loss = loss.clone()
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=self.group)
            probs, y = self._gather(probs), self._gather(y_local.to(probs.device))
        return loss, probs, y

    def _gather(self, t):
        parts = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(parts, t.contiguous(), group=self.group)
        return torch.cat(parts, dim=0)


# ---------------------------------------------------------------------------------------------------- the epoch driver (:24-220)
def reference_schedule():
    """MainParallel.py:74-75."""
    from .schedules import PiecewiseConstantDecay
    return PiecewiseConstantDecay([10000, 20000, 40000, 60000, 80000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])


class Process(object):
    """MainParallel.py:24-176 (module docstring).  ``history``: one dict per training epoch (``phase`` "train") and per ``test`` call
    (``phase`` "test"), the same on every rank."""

    def __init__(self, batch_size=16, *, schedule=False, capture_graph=True, group=None):
        self.batch_size = batch_size
        self.input_shape = [256, 80, 10]                                                           # :29
        self.schedule, self.capture_graph, self.group = schedule, capture_graph, group
        self.train_iter = 0
        self.test_iter = 0
        self.history = []
        self.trainer = None

    def _mirror(self, neuralnet) -> MirroredTrainer:
        """Wrap the model once (rank-0 broadcast, gradient exchange) and make its counters: precision / recall / pre_c2 / re_c2 / mio
        (:30-34) and tr_recall / tr_precision / tr_mio (:35-37)."""
        if self.trainer is None or self.trainer.net is not neuralnet:
            from .metrics import SegMetrics
            self.trainer = MirroredTrainer(neuralnet, self.group)
            self.metrics = SegMetrics(3, round=True, device=neuralnet.device)
            self.tr_metrics = SegMetrics(3, round=True, device=neuralnet.device)
            self._zero = torch.zeros((), dtype=torch.float32, device=neuralnet.device)
        return self.trainer

    def _print(self, *args, **kwargs):
        if self.trainer is None or self.trainer.rank == 0:
            print(*args, **kwargs)

    def training(self, neuralnet, dataset, epochs, batch_size, *, boundary_ramp=None):
        """MainParallel.py:41-79 -> None.  ``boundary_ramp`` (default off): added to the model's boundary
        weight after each epoch - Kervadec et al.'s rebalancing; the weight is a device float, so a captured graph follows it."""
        assert batch_size == self.batch_size == dataset.BATCH_SIZE, "one global batch size for the driver, the dataset and the model"
        self._mirror(neuralnet)
        self._print("\nTraining to %d epochs (%d of minibatch size)" % (epochs, batch_size))
        if self.schedule:
            from .MainNumpy import install_schedule
            install_schedule(neuralnet, reference_schedule(), lr_scale=1e-3, wd_scale=1e-4)      # :74-79, once (module docstring)
        prev_loss = 0
        for epoch in range(epochs):
            if neuralnet.optimizer.current_learning_rate() < 1e-5:                                # :49
                break
            loss = self.mirrored_train_step(neuralnet, dataset)                                  # :52-60
            self._print()
            m = self.tr_metrics.result()
            self._print("Epoch [%d / %d] (%d iteration)  Loss:%.5f, Recall:%.5f, Precision:%.5f, IoU:%.5f"
                        % (epoch, epochs, self.train_iter, loss, m["recall"], m["precision"], m["mean_iou"]))
            self.history.append(dict(m, phase="train", epoch=epoch, iteration=self.train_iter, loss=loss))
            self.tr_metrics.reset_states()                                                       # :66-68
            self._paste_report(dataset)
            if prev_loss == loss:
                self._print("Model is throwing a fit")
            prev_loss = loss
            if boundary_ramp is not None:
                neuralnet.set_boundary_weight(neuralnet.boundary_weight + float(boundary_ramp))
            self.test(neuralnet, dataset, epoch)                                                 # :72

    def _paste_report(self, dataset):
        """With ``paste=``: the epoch's line on rank 0.  Every rank drew the lesions of the whole global batches, so ``drawn`` is the same
        everywhere; the device counters hold the rank's own slices and are SUM-reduced before the one read-back."""
        if getattr(dataset, "paste", None) is None:
            return None
        if self.trainer is not None and self.trainer.world > 1:
            dist.all_reduce(dataset.paste_counts, op=dist.ReduceOp.SUM, group=self.group)
        from .MainNumpy import paste_report
        return paste_report(dataset, show=self._print)

    def test(self, neuralnet, dataset, epoch):
        """MainParallel.py:81-115 -> F1 of the test set; its dict (``phase`` "test") is appended to ``history``.  A model built with
        ``average=`` is tested under ``averaged_weights()`` (every rank holds the same average: same weights, same counter); the report adds
        the loss of the raw weights (``raw_loss`` in the history)."""
        self._mirror(neuralnet)
        self._print("\nTest...")
        averaged = averaging(neuralnet)
        extra = {}
        if averaged:
            extra["raw_loss"] = self.mirrored_test_step(neuralnet, dataset)                      # the weights as they stand, for comparison
            self.metrics.reset_states()
        with (neuralnet.averaged_weights() if averaged else contextlib.nullcontext()):
            total_loss = self.mirrored_test_step(neuralnet, dataset)                             # :86, not divided (:89)
        m = self.metrics.result()
        self._print("loss = {}".format(total_loss))
        if averaged:
            self._print("loss (raw weights) = {}".format(extra["raw_loss"]))
        self._print("IoU = {}".format(m["mean_iou"]))
        self._print("f1 = {}".format(m["f1"]))
        self._print("precision = {}".format(m["precision"]))
        self._print("recall = {}".format(m["recall"]))
        dice = dice_line(neuralnet, self.metrics)
        if dice is not None:                                    # only with loss="dice" / "tversky" / "dice_ce"
            self._print("dice per class = {}".format(dice))
        terms = distill_line(neuralnet)
        if terms is not None:                                   # only with loss="distill": this replica's last validation batch, one read-back an epoch
            self._print("distill terms: {}".format(terms))
        self.history.append(dict(m, phase="test", epoch=epoch, loss=total_loss, **extra))
        self.metrics.reset_states()                                                              # :110-114
        return m["f1"]

    def save(self, neuralnet, path) -> bool:
        """``visionModel.save(path)`` on rank 0 only (MainParallel.py:216; every rank holds the same weights) -> whether this rank saved.
        A model built with ``average=`` also writes ``<path>.avg``, a plain checkpoint of the averaged weights (``save_averaged``)."""
        rank = dist.get_rank(self.group) if dist.is_initialized() else 0
        if rank == 0:
            neuralnet.visionModel.save(path)
            if averaging(neuralnet):
                neuralnet.save_averaged(path + ".avg")
        return rank == 0

    def mirrored_train_step(self, neuralnet, dataset) -> float:
        """MainParallel.py:117-146: one epoch of this replica's slices -> the last step's SUM-reduced loss.  The training counters are
        SUM-reduced once at the end."""
        tr = self._mirror(neuralnet)
        local = self.batch_size // tr.world                                                      # images of a full local batch
        last = self._zero
        for x, y, _ in dataset.train_batches(tr.rank, tr.world):
            if x is None:
                neuralnet.empty_step()                                                           # joins the exchange: no deadlock
                last = self._zero
            else:
                if self.capture_graph and getattr(neuralnet, "_graph", None) is None and x.shape[0] == local:
                    neuralnet.capture_graph(x, y)
                last, class_score = neuralnet.train_step(x, y)                                   # :130
                self.tr_metrics.update_state(y, class_score)
            self.train_iter += 1
            self._print('.', end='')
            if (self.train_iter + 1) % 100 == 0:
                self._print()
        flush(neuralnet)     # accumulate=N: a short last group still takes its optimiser step (every rank holds the same count: one more exchange)
        loss = last.detach().reshape(()).clone()         # after a replay ``last`` is the step's static buffer, still this last step's
        if tr.world > 1:
            dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=self.group)                        # :131
            self.tr_metrics.reduce(self.group)
        return float(loss)

    def mirrored_test_step(self, neuralnet, dataset) -> float:
        """MainParallel.py:148-176: the test set in batches of ``batch_size`` (:155) -> the sum of the batch losses (:170).  The loss
        and the counters are summed on the device and SUM-reduced once (the reference gathers probabilities and labels, :160,163)."""
        tr = self._mirror(neuralnet)
        total = self._zero.clone()
        for x, y, _ in dataset.test_batches(tr.rank, tr.world):
            if x is not None:
                loss, class_score = neuralnet.step(x, y)                                         # :158
                total.add_(loss.reshape(()))
                self.metrics.update_state(y, class_score)                                        # :162-169
            self.test_iter += 1
        if tr.world > 1:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)                       # :159
            self.metrics.reduce(self.group)
        return float(total)


def main(train_path, val_path, save_path=None, epochs=51, batch_size=64, use_vit=True, *, seed=0, schedule=False, capture_graph=True,
         loss="cce", overlap=None, boundary=None, lovasz=None, average=None, warp=None, topk=None, teacher=None, distill=None,
         teacher_use_vit=None, teacher_flip=False, accumulate=None, paste=None):
    """MainParallel.py:201-216 with the paths as arguments: ``VisionTransformer(batch_size=64)`` with the ViT bottleneck, 51 epochs,
    then rank 0 saves if ``save_path`` is given.  Every rank seeds ``random`` with ``seed``, so all draw the same augmentations.
    ``loss``: the model's ``loss=`` ("cce", "my_loss_cat", "focal"); every replica divides it by the global batch all the same.  The
    region-overlap losses ("dice", "tversky", "dice_ce", settings in ``overlap``) are computed per replica on its own images and weighted by
    local batch / global batch: the SUM of the replicas is their batch-weighted mean; they add a per-class Dice line to the test report.
    ``boundary`` (``VisionTransformer(boundary=...)``) adds the boundary term to one of those three, weighted per replica the same way.
    The Lovasz-softmax loss ("lovasz", "lovasz_ce", settings in ``lovasz``) ranks the pixels of the images a replica holds and is weighted like the
    overlap term; it adds the Dice line too.
    The top-k cross-entropy ("topk", "dice_topk", settings in ``topk``): with scope "batch" a replica selects among the pixels of the images it holds,
    with scope "image" the selection is per image and does not depend on how the batch is split; every replica divides by the global batch all
    the same, and the Dice term of "dice_topk" is weighted like the overlap term.  The Dice line too.
    Knowledge distillation ("distill", settings in ``distill``): ``teacher`` is a model, an ``Ensemble``, or checkpoint paths (a list or a
    comma-separated string; several, or ``teacher_flip``, make an ensemble; ``teacher_use_vit`` says whether they have the ViT bottleneck,
    default: as the student).  Every replica holds its own copy of the teacher, which sees the replica's slice of the batch; the loss is
    divided by the global batch all the same, so the SUM of the replicas is the batch's loss.  The test report adds the two terms.
    ``average`` (a dict, or the ``--average`` string ``ema:DECAY[:dynamic]`` / ``swa:START:PERIOD``): EMA / SWA weight averaging; the update of
    every rank keeps the same average (no exchange is added), the tests report the averaged model and rank 0 also saves ``<save_path>.avg``.
    ``warp`` (a ``warp.warp_config`` dict or the ``--warp`` string; default off): elastic / affine warp of every training batch ahead of ``dataAug``;
    its draws come from ``random.Random(seed)`` on every rank, each rank draws the whole global batch and keeps its slice.
    ``accumulate`` (``--accumulate N``; None: 1): every global batch is a micro-batch and N of them make one optimiser step - ONE gradient exchange
    and one update per N batches; a short last group of an epoch is flushed before the test and the save.
    ``paste`` (a ``paste.paste_config`` dict or the ``--paste`` string; default off): lesions of the training set are pasted into every training
    batch ahead of the warp; its draws come from ``random.Random(seed)`` on every rank, each rank draws the whole global
    batch and keeps its slice, and rank 0 prints one line per epoch: lesions placed of lesions drawn, summed over the ranks.
    Under ``nccl`` the model lives on ``cuda:LOCAL_RANK``; the ``USSEG_DIST_BACKEND=gloo`` rehearsal keeps every rank on device 0."""
    from .Dataset import Dataset
    from .MainNumpy import average_setting
    from .VisionTransformer import VisionTransformer, overlap_settings
    rank, world, local = init_distributed()
    nccl = world > 1 and dist.get_backend() == "nccl"
    device = torch.device("cuda", local if nccl else 0)
    torch.cuda.set_device(device)
    random.seed(seed)
    dataset = Dataset(train_path, val_path, batch_size, device=device, warp=warp, warp_seed=seed, paste=paste, paste_seed=seed)
    kw = {} if topk is None else {"topk": topk}
    if teacher is not None or distill is not None:
        if isinstance(teacher, (str, list, tuple)):
            from .distill import load_teacher
            teacher = load_teacher(teacher, (dataset.height, dataset.width), dataset.channel, device,
                                   use_vit=use_vit if teacher_use_vit is None else teacher_use_vit, flip=teacher_flip)
        kw.update(teacher=teacher, distill=distill)
    neuralnet = VisionTransformer(batch_size, img_size=(dataset.height, dataset.width), in_channels=dataset.channel, use_vit=use_vit,
                                  device=str(device), loss=loss, overlap=overlap_settings(loss, overlap), boundary=boundary, lovasz=lovasz,
                                  average=average_setting(average), accumulate=accumulate, **kw)
    if rank == 0:
        print(len(neuralnet.visionModel.layers))
    process = Process(batch_size, schedule=schedule, capture_graph=capture_graph)
    process.training(neuralnet=neuralnet, dataset=dataset, epochs=epochs, batch_size=batch_size)
    if save_path is not None:
        process.save(neuralnet, save_path)                                                       # :216
    return neuralnet, process


def _cli(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ultrasound_modeling_amd.MainParallel",
                                 description="Data-parallel training of the VisionTransformer (MainParallel.py); launch N ranks with "
                                             "torch.distributed.run, or run world size 1 directly.")
    ap.add_argument("train", help="training .npy [N,1,H,W,12]")
    ap.add_argument("val", help="validation .npy [N,1,H,W,12]")
    ap.add_argument("--save", default=None, help="rank 0 saves the model here after training")
    ap.add_argument("--epochs", type=int, default=51)
    ap.add_argument("--batch-size", type=int, default=64, help="GLOBAL batch, divided evenly over the ranks")
    ap.add_argument("--no-vit", action="store_true", help="the conv-only model (no ViT bottleneck)")
    ap.add_argument("--seed", type=int, default=0, help="augmentation draws (the same on every rank)")
    ap.add_argument("--schedule", action="store_true", help="install the MainParallel.py:74-79 rate schedule once")
    ap.add_argument("--no-graph", action="store_true", help="run every step eagerly")
    ap.add_argument("--loss", choices=("cce", "my_loss_cat", "focal", "dice", "tversky", "dice_ce") + ("lovasz", "lovasz_ce") + ("topk", "dice_topk") + ("distill",), default="cce",
                    help="the model's loss: CategoricalCrossentropy (the reference's), its class-weighted my_loss_cat, the focal variant, or a "
                         "region-overlap loss (soft Dice, Tversky 0.3 / 0.7, Dice + CCE), or the Lovasz-softmax loss (alone, or CCE + it), or the "
                         "top-k cross-entropy (alone, or soft Dice + it), or knowledge distillation from --teacher")
    ap.add_argument("--teacher", default=None, metavar="CKPT[,CKPT...]",
                    help="the teacher checkpoint(s) of --loss distill; more than one, or --teacher-flip, makes an ensemble whose mean is the teacher")
    ap.add_argument("--teacher-use-vit", action="store_true", help="the teacher checkpoints have the ViT bottleneck (default: as the student)")
    ap.add_argument("--teacher-flip", action="store_true", help="add the left-right mirrored view of every teacher member")
    ap.add_argument("--distill-temperature", type=float, default=None, metavar="T", help="the softening temperature in [1/8, 8] (default 2)")
    ap.add_argument("--distill-soft-weight", type=float, default=None, metavar="A", help="the weight of the soft term (default 0.5)")
    ap.add_argument("--distill-hard-weight", type=float, default=None, metavar="B", help="the weight of the label term (default 0.5)")
    ap.add_argument("--topk-fraction", type=float, default=None, metavar="F",
                    help="the fraction of the pixels with the largest loss that --loss topk / dice_topk averages over, in (0, 1] (default 0.1)")
    ap.add_argument("--topk-scope", choices=("batch", "image"), default=None,
                    help="select among all the pixels a replica holds (batch, the default) or within each image (image)")
    ap.add_argument("--boundary-weight", type=float, default=None, metavar="W",
                    help="add the boundary term (signed distance map of the labels times the probabilities) with weight W; needs a region-overlap --loss")
    ap.add_argument("--average", default=None, metavar="ema:DECAY[:dynamic] | swa:START:PERIOD",
                    help="keep an EMA or SWA average of the weights inside the optimiser step; the tests report the averaged model and "
                         "--save also writes SAVE.avg with the averaged weights")
    ap.add_argument("--accumulate", type=int, default=None, metavar="N",
                    help="gradient accumulation: N global batches (micro-batches) per optimiser step - one gradient exchange and one update per N")
    ap.add_argument("--warp", default=None, metavar="SPEC",
                    help="warp every training batch elastically and affinely on the device before dataAug, e.g. "
                         "sigma=8,magnitude=2:1,p=0.5,rotate=5,scale=0.05,shift=0:0 (any subset; these are the defaults)")
    ap.add_argument("--paste", default=None, metavar="SPEC",
                    help="paste lesions of the training set into every training batch on the device, before the warp and dataAug, e.g. "
                         "p=0.5,max_lesions=2,min_area=4,min_landed=0.5,flip=1,shift=none,protect=1,connectivity=8 (any subset; these are "
                         "the defaults, whose effect on this data nobody has measured)")
    a = ap.parse_args(argv)
    if a.paste is not None:
        from .paste import parse_paste
        try:
            parse_paste(a.paste)
        except ValueError as e:
            raise SystemExit(str(e))
    if a.warp is not None:
        from .warp import parse_warp
        try:
            parse_warp(a.warp)
        except ValueError as e:
            raise SystemExit(str(e))
    if a.accumulate is not None:
        from .flat import accumulate_config
        try:
            accumulate_config(a.accumulate)
        except ValueError as e:
            raise SystemExit(str(e))
    if a.average is not None:
        from .flat import parse_average
        try:
            parse_average(a.average)
        except ValueError as e:
            raise SystemExit(str(e))
    if a.boundary_weight is not None and a.loss not in ("dice", "tversky", "dice_ce"):
        raise SystemExit("--boundary-weight needs --loss dice, tversky or dice_ce")
    topk = {k: v for k, v in (("fraction", a.topk_fraction), ("scope", a.topk_scope)) if v is not None}
    if topk and a.loss not in ("topk", "dice_topk"):
        raise SystemExit("--topk-fraction / --topk-scope need --loss topk or dice_topk")
    if "fraction" in topk:
        from . import ops
        try:
            ops.topk_fraction_value(topk["fraction"])
        except ValueError as e:
            raise SystemExit(str(e))
    dst = {k: v for k, v in (("temperature", a.distill_temperature), ("soft_weight", a.distill_soft_weight), ("hard_weight", a.distill_hard_weight))
           if v is not None}
    if (dst or a.teacher or a.teacher_use_vit or a.teacher_flip) and a.loss != "distill":
        raise SystemExit("--teacher / --teacher-use-vit / --teacher-flip / --distill-* need --loss distill")
    dkw = {}
    if a.loss == "distill":
        if not a.teacher:
            raise SystemExit("--loss distill needs --teacher CKPT[,CKPT...]")
        from .distill import distill_config
        try:
            distill_config(dst)
        except ValueError as e:
            raise SystemExit(str(e))
        dkw = dict(teacher=a.teacher, distill=dst, teacher_use_vit=True if a.teacher_use_vit else None, teacher_flip=a.teacher_flip)
    main(a.train, a.val, a.save, epochs=a.epochs, batch_size=a.batch_size, use_vit=not a.no_vit, seed=a.seed, schedule=a.schedule,
         capture_graph=not a.no_graph, loss=a.loss, boundary=None if a.boundary_weight is None else {"weight": a.boundary_weight},
         average=a.average, warp=a.warp, accumulate=a.accumulate, paste=a.paste, **({"topk": topk} if topk else {}), **dkw)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    _cli()
