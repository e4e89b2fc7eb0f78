"""The order of one optimisation step, shared by both model wrappers (VisionTransformer.py:235-246; TBI_ResNest.py:35-55)
and by the data-parallel path (MainParallel.py:117-146).

    zero gradients -> forward -> loss -> backward            (tape, VisionTransformer.py:237-243)
    [data parallel] per-replica clip-by-global-norm          (:244 - it precedes :245, so every replica clips ITS OWN gradient)
    [data parallel] SUM all-reduce of the flat gradient      (apply_gradients under MirroredStrategy, :245 / MainParallel.py:130)
    clip (single replica only) + Adam                        (:244-245)
    rebuild the bf16 GEMM operands from the fp32 masters

With gradient accumulation (``optimizer.accumulate_steps`` = N > 1; not in the reference) the first line is a
MICRO-STEP, followed by ``optimizer.accumulate(finish)``: N - 1 micro-steps add their gradient to the accumulator and stop there; the N-th
leaves the mean of the N gradients in ``flat.grad`` and the rest of the order runs on it unchanged, once per N micro-batches.

This file is host logic only (no kernel is launched from here directly): a wrapper supplies three hooks
(``_zero_grad``, ``_forward_backward``, ``_repack``) and an ``optimizer`` with ``clip_local / advance / apply / apply_range``
(and ``accumulate`` when it accumulates).
That makes the ordering testable on CPU with gloo (tests/test_cpu_host.py drives THIS class with oracle arithmetic in the
hooks) and on one GPU with an in-process RCCL group (tests/test_gpu_step.py).

HIP-graph replay: the whole step is captured once per input shape and replayed (one graph; with a gradient exchange the
step is one graph up to the per-replica clip, the collective, then the update).
"""
from __future__ import annotations

import contextlib
from typing import Callable, Iterable, List, Optional, Tuple

import torch


class TrainStepDriver:
    grad_sync: Optional[Callable] = None     # set by MainParallel.MirroredTrainer: callable(flat_grad) [+ .chunks(flat_grad)]
    _graph = None

    # ------------------------------------------------------------------ hooks a wrapper implements
    def _zero_grad(self):
        raise NotImplementedError

    def _forward_backward(self, x, y):
        """forward, loss, backward: parameter gradients accumulated into ``flat.grad``; -> probabilities."""
        raise NotImplementedError

    def _repack(self):
        raise NotImplementedError

    def _graph_state(self) -> List[torch.Tensor]:
        """Tensors that the capture warm-up steps modify and ``capture_graph`` must put back (weights, Adam state, BN statistics)."""
        return []

    # ------------------------------------------------------------------ gradient accumulation (flat.AdamClip(accumulate=N))
    _pending = 0             # host counter: micro-steps of the current group that are in the accumulator
    _graph_micro = None      # the captured micro-step (``capture_graph`` with accumulate > 1), beside ``_graph``

    @property
    def accumulate(self) -> int:
        """Micro-batches per optimiser step (1: every ``train_step`` is an optimiser step)."""
        return getattr(self.optimizer, "accumulate_steps", 1)

    @property
    def pending_micro_steps(self) -> int:
        """Micro-steps taken since the last optimiser step; ``flush_step()`` (or N - k more micro-steps) puts it back to 0."""
        return self._pending

    def _finishes(self) -> bool:
        """Whether the micro-step about to run is the last of its group."""
        return self._pending + 1 >= self.accumulate

    def _micro_body(self, x, y):
        """A micro-step that does not finish its group: no clip, no exchange, no Adam, no repack, no step-counter advance."""
        self._zero_grad()
        probs = self._forward_backward(x, y)
        self.optimizer.accumulate(False)
        return probs

    def _finish_empty(self):
        """The finishing micro-step of a replica that holds no image (``empty_step``) or of a short group (``flush_step``): a zero gradient
        into the accumulator, then the tail of the step - through the captured update graph where there is one."""
        self._zero_grad()
        if self.accumulate > 1:
            self.optimizer.accumulate(True)
        self._pending = 0
        if self.grad_sync is None:
            self._update_body()
            return
        self.optimizer.clip_local()
        g2 = None if self._graph is None else self._graph[1]
        if g2 is not None:
            self.grad_sync(self.flat.grad)
            g2.replay()
        else:
            self._sync_and_update()

    def flush_step(self):
        """Finishes a group of k < N pending micro-steps with one optimiser step on (their sum) / N - the reference divides a short last
        batch by the constant global batch size in the same way.  Nothing pending: nothing happens.  Under a ``grad_sync`` every replica
        calls it (they hold the same count)."""
        if self._pending == 0:
            return
        self._not_averaged()
        self._finish_empty()

    def _no_pending(self, what: str):
        if self._pending:
            raise RuntimeError(f"{what}: {self._pending} of {self.accumulate} micro-steps are pending in the gradient accumulator, which a "
                               f"checkpoint does not hold; call flush_step() first")

    # ------------------------------------------------------------------ the step
    def _grad_body(self, x, y):
        """The micro-step that ends in an optimiser step (with ``accumulate`` 1: every step)."""
        self._zero_grad()
        probs = self._forward_backward(x, y)                       # :240-243
        if self.accumulate > 1:
            self.optimizer.accumulate(True)                        # flat.grad = the mean of the group's gradients
        if self.grad_sync is not None:
            self.optimizer.clip_local()                            # per-replica clip (:244) BEFORE the exchange
        return probs

    def _update_body(self):
        self.optimizer.apply(already_clipped=self.grad_sync is not None)      # (:244-)245 clip + Adam
        self._repack()

    def _sync_and_update(self):
        """Gradient exchange + update.  A ``grad_sync`` with ``chunks`` pipelines the exchange: chunk k+1 is on the wire
        (RCCL's stream) while the Adam kernel of chunk k runs - exact, because after the per-replica clip both the SUM and
        the Adam update are elementwise over the flat buffer."""
        gs = self.grad_sync
        chunks = getattr(gs, "chunks", None)
        if chunks is None:
            gs(self.flat.grad)
            self._update_body()
            return
        self.optimizer.advance()
        for lo, hi, wait in chunks(self.flat.grad):
            wait()
            self.optimizer.apply_range(lo, hi)
        self._repack()

    def _step_body(self, x, y):
        probs = self._grad_body(x, y)
        if self.grad_sync is not None:
            self._sync_and_update()
        else:
            self._update_body()
        return probs

    def _train_body(self, x, y):
        self._not_averaged()
        if not self._finishes():
            probs = self._micro_body(x, y)
            self._pending += 1
            return probs
        probs = self._step_body(x, y)
        self._pending = 0
        return probs

    def empty_step(self):
        """This replica's part of a step in which it holds no image (a short last batch split over the replicas): no forward pass and
        so no BatchNorm-statistics update, a zero gradient, and the same exchange and update as every other replica - the collective is
        joined, so no rank waits on it, and the weights stay identical.  The per-replica clip of a zero gradient is a no-op
        (scale = clip / max(0, clip) = 1), so the replica adds exactly nothing to the sum.  With a captured step the update replays
        the captured update graph; a single replica (no ``grad_sync``) takes one Adam step on the zero gradient.
        With gradient accumulation it counts as a micro-step: a zero gradient into the accumulator, and the update only as the N-th."""
        self._not_averaged()
        if not self._finishes():
            self._zero_grad()
            self.optimizer.accumulate(False)
            self._pending += 1
            return
        self._finish_empty()

    # ------------------------------------------------------------------ the averaged weights (flat.AdamClip(average=...))
    _averaged = False

    def _not_averaged(self):
        if self._averaged:
            raise RuntimeError("a training step inside averaged_weights(): the weight buffer holds the averages; leave the block first")

    @contextlib.contextmanager
    def averaged_weights(self, repack: bool = True):
        """Inside the block the model computes with the optimiser's averaged weights (EMA / SWA): ``flat.flat`` and ``optimizer.avg`` are
        exchanged IN PLACE (``AdamClip.swap_average``) and the bf16 GEMM operands rebuilt, and exchanged back on the way out.  No pointer changes, so
        captured training and predict graphs stay valid, and a predict graph replayed inside the block reads the averaged operands.
        BatchNorm moving statistics are NOT averaged (tfa averages trainable variables only): inside the block they are the raw model's.
        A training step inside the block raises.  ``repack=False`` skips both operand rebuilds (for reading the fp32 weights only)."""
        opt = self.optimizer
        if getattr(opt, "avg", None) is None:
            raise ValueError("averaged_weights: the model was built without average=")
        if self._averaged:
            raise RuntimeError("averaged_weights: already inside the block")
        opt.swap_average()
        if repack:
            self._repack()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            opt.swap_average()
            if repack:
                self._repack()

    def save_averaged(self, path):
        """A plain checkpoint whose variables are the averaged weights (BatchNorm statistics as they are, no optimiser state): every loader
        of a model file reads it with no new knowledge - ``load``, the evaluator's ``--bleed`` / ``--bleed-extra``, ``Cascade``, ``Ensemble``."""
        with self.averaged_weights(repack=False):
            d = self.export_params()
        torch.save(d, path)

    # ------------------------------------------------------------------ HIP-graph replay of the whole step
    def capture_graph(self, x, y, warmup: int = 2):
        """Capture the training step for inputs of this shape.  The ``warmup`` eager steps it needs (workspaces grow, lazy
        tables are built) run on a throw-away copy of the training state: weights, Adam moments / step counter and BatchNorm
        statistics are restored afterwards, so enabling the graph does not consume optimisation steps.
        With gradient accumulation two steps are captured, each warmed up: the micro-step (one graph) and the step that finishes a group (the
        graphs below); the accumulator is part of the restored state and the host counter of pending micro-steps is not touched, so a
        capture in the middle of a group leaves the group as it was.  ``train_step`` replays whichever the counter calls for."""
        self._not_averaged()
        x, y = self._prep_x(x), self._prep_y(y)
        self._gx, self._gy = x.clone(), y.clone()
        state = self._graph_state()
        saved = [t.clone() for t in state]
        sync_saved = self.grad_sync
        self.grad_sync = None if sync_saved is None else _LocalSync()      # no collective during the warm-up (ranks stay in step)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                if self.accumulate > 1:
                    self._micro_body(self._gx, self._gy)
                self._step_body(self._gx, self._gy)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.grad_sync = sync_saved
        for t, v in zip(state, saved):
            t.copy_(v)
        self._repack()
        torch.cuda.synchronize()
        mark = getattr(self.optimizer, "mark_captured", None)
        if mark is not None:
            mark()                    # the optimiser's kernel path is now part of the graph (flat.AdamClip)
        g1, pool = torch.cuda.CUDAGraph(), {}
        self._graph_micro = None
        if self.accumulate > 1:       # the micro-step: its own graph and probability buffer, the memory pool shared with the graphs below
            self._graph_micro = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph_micro):
                self._gprobs_micro = self._micro_body(self._gx, self._gy)
            pool = {"pool": self._graph_micro.pool()}
        if self.grad_sync is None:
            with torch.cuda.graph(g1, **pool):
                self._gprobs = self._step_body(self._gx, self._gy)
            self._graph = (g1, None)
            return
        with torch.cuda.graph(g1, **pool):
            self._gprobs = self._grad_body(self._gx, self._gy)
        g2 = None
        if getattr(self.grad_sync, "chunks", None) is None:          # one collective -> the update is a second graph
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=g1.pool()):
                self._update_body()
        self._graph = (g1, g2)

    def graph_inputs(self):
        """The (x, y) buffers the captured step reads: write the next batch THERE and pass these tensors to ``train_step`` - no copy."""
        return self._gx, self._gy

    def _graph_takes(self, x, y) -> bool:
        """True when the captured step can run on (x, y): the shape, dtype, strides and device of the buffers it was captured with.
        Any other input (a short last batch) runs eagerly - a copy into the captured buffers would broadcast or fail."""
        if self._graph is None:
            return False
        return all(a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride() and a.device == b.device
                   for a, b in ((x, self._gx), (y, self._gy)))

    def _graph_replay(self, x, y):
        """-> the STATIC probability buffer of the captured step (overwritten by the next replay)."""
        # a producer that writes the batch straight into the captured step's input buffers (``graph_inputs()``: the device input
        # pipeline, a data loader with pinned staging) skips these two copies
        self._not_averaged()
        if x.data_ptr() != self._gx.data_ptr():
            self._gx.copy_(x)
        if y.data_ptr() != self._gy.data_ptr():
            self._gy.copy_(y)
        if not self._finishes():      # a micro-step inside a group: the probabilities are those of the micro-batch just run
            self._graph_micro.replay()
            self._pending += 1
            return self._gprobs_micro
        self._pending = 0
        g1, g2 = self._graph
        g1.replay()
        if self.grad_sync is not None:
            if g2 is not None:
                self.grad_sync(self.flat.grad)
                g2.replay()
            else:
                self._sync_and_update()
        return self._gprobs


class PredictDriver:
    """Label-free inference, eager or replayed from a captured forward-only HIP graph.  A wrapper supplies ``_prep_x``,
    ``_predict_body(x) -> probabilities`` (no loss, no gradient, no optimiser or BatchNorm-statistics write) and optionally
    ``_predict_state()``: device tensors a predict call advances (a dropout counter) that the capture warm-up must put back."""
    _pgraph = None

    def _predict_body(self, x):
        raise NotImplementedError

    def _predict_state(self) -> List[torch.Tensor]:
        return []

    def predict(self, x):
        """x [B,H,W,C] (numpy or tensor) -> fp32 probabilities [B,H,W,classes].  After ``capture_predict_graph`` an input with the captured
        shape, dtype and strides is copied into ``predict_inputs()`` (no copy if it already is that buffer) and the graph is replayed: the
        result is then the graph's STATIC probability buffer, valid until the next call (clone it to keep it).  Any other input runs eagerly."""
        x = self._prep_x(x)
        px = getattr(self, "_px", None)
        if self._pgraph is not None and x.dtype == px.dtype and x.shape == px.shape and x.stride() == px.stride() and x.device == px.device:
            if x.data_ptr() != px.data_ptr():
                px.copy_(x)
            self._pgraph.replay()
            return self._pprobs
        return self._predict_body(x)

    def capture_predict_graph(self, x, warmup: int = 2):
        """Capture one forward-only HIP graph of ``predict`` for inputs of this shape, dtype and strides.  The eager warm-up calls run
        on a side stream and the predict state they advance is restored, so capturing consumes no dropout draws; training state is
        never touched.  Coexists with a captured training step (``capture_graph``) in either order."""
        x = self._prep_x(x)
        self._px = x.clone()
        state = self._predict_state()
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._predict_body(self._px)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for t, v in zip(state, saved):
            t.copy_(v)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._pprobs = self._predict_body(self._px)
        self._pgraph = g

    def _norm_layers(self) -> list:
        """The layers with a ``training_mode`` switch (BatchNormalization), listed once: ``inference_norms`` takes them."""
        if getattr(self, "_pnorms", None) is None:
            self._pnorms = [m for m in self.modules() if hasattr(m, "training_mode")]
        return self._pnorms

    def predict_inputs(self):
        """The input buffer the captured predict graph reads: write the next batch THERE and pass it to ``predict`` - no copy."""
        return self._px


@contextlib.contextmanager
def inference_norms(modules: Iterable):
    """BatchNormalization layers in batch-statistics mode run on their moving statistics (Keras ``training=False``) inside the block,
    so a predict call neither reads the batch's statistics nor moves the running ones."""
    bns = [m for m in modules if getattr(m, "training_mode", False)]
    for m in bns:
        m.training_mode = False
    try:
        yield
    finally:
        for m in bns:
            m.training_mode = True


class _LocalSync:
    """Stands in for the exchange during graph warm-up: the data-parallel code path (clip_local, already-clipped Adam)
    without a collective."""

    def __call__(self, flat_grad):
        return None


def even_chunks(n: int, k: int, align: int = 1024) -> List[Tuple[int, int]]:
    """Split [0, n) into <= k contiguous ranges whose boundaries are multiples of ``align`` (the last one takes the tail)."""
    k = max(1, min(k, max(1, n // align)))
    per = (n + k - 1) // k
    per = (per + align - 1) // align * align
    out, lo = [], 0
    while lo < n:
        hi = min(n, lo + per)
        out.append((lo, hi))
        lo = hi
    return out
