"""Flat parameter / gradient storage and the clip-by-global-norm + Adam step.

All trainable variables of a model live in ONE fp32 device buffer (and their gradients, Adam moments in
three more of the same shape), so that
  * the global gradient norm, the clip and the Adam update are one kernel each
    (VisionTransformer.py:244-245; TBI_ResNest.py:46),
  * the data-parallel gradient exchange is ONE RCCL all-reduce over the flat gradient buffer
    (MainParallel.py:130 -> apply_gradients under MirroredStrategy),
  * kernels accumulate parameter gradients straight into the flat gradient buffer.
Every variable starts on a 32-byte boundary and is followed by zero padding up to a multiple of 8 floats, so
kernels may read per-channel vectors up to the physical (padded) channel count.  Modules may ask for several
variables to be laid out back to back ("adjacent groups", used by the grouped split-attention kernels).
"""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .schedules import MAX_PIECES, PiecewiseConstantDecay


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


class FlatParams:
    def __init__(self, module: nn.Module, device):
        self.device = torch.device(device)
        named = list(module.named_parameters())
        self.names = [n for n, _ in named]
        params = [p for _, p in named]
        pid = {id(p): i for i, p in enumerate(params)}
        offsets: Dict[int, int] = {}
        off = 0
        # adjacency groups first
        for m in module.modules():
            fn = getattr(m, "adjacent_params", None)
            if fn is None:
                continue
            for group, extra_pad in fn():
                for p in group:
                    assert id(p) in pid and id(p) not in offsets, "parameter in two adjacency groups"
                    offsets[id(p)] = off
                    off += p.numel()
                off = _pad8(off + extra_pad)
        for p in params:
            if id(p) in offsets:
                continue
            offsets[id(p)] = off
            off = _pad8(off + p.numel())
        self.total = _pad8(off)
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros_like(self.flat)
        self.params = params
        self.offsets = [offsets[id(p)] for p in params]
        for p, o in zip(params, self.offsets):
            n = p.numel()
            view = self.flat[o:o + n].view(p.shape)
            view.copy_(p.data.to(torch.float32))
            p.data = view
            p.requires_grad_(False)
            p.grad = self.grad[o:o + n].view(p.shape)
        for m in module.modules():
            for k, b in list(m._buffers.items()):
                if b is not None:
                    m._buffers[k] = b.to(self.device)
        self.n_trainable = sum(p.numel() for p in params)
        for m in module.modules():
            fn = getattr(m, "on_finalize", None)
            if fn is not None:
                fn(self.device)

    def zero_grad(self):
        ops.fill_f32(self.grad, 0.0)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {n: p.data.detach().clone() for n, p in zip(self.names, self.params)}


class AdamClip:
    """tf.clip_by_global_norm(grads, clip) followed by tf.optimizers.Adam(lr) (Keras defaults: b1 .9, b2 .999, eps 1e-7).

    ``clip_norm=None`` disables clipping (TBI_ResNest.py:46 applies raw gradients).
    The step counter and the bias-corrected learning rate live on the device so that a captured HIP graph of the
    whole training step can be replayed.

    ``lr`` and ``weight_decay`` may each be a float or a ``schedules.PiecewiseConstantDecay``.  ``weight_decay`` (None: off) is tfa's
    DecoupledWeightDecayExtension (AdamW): ``p -= wd_t * p`` before the Adam update, not scaled by the learning rate.
    ``decay_exclude`` (regexes searched in ``FlatParams.names``) keeps matching variables out of the decay.  With a schedule or a
    decay the rates come from a device table (``UssegLrSchedule``) read at the device step counter by the step kernels, so
    ``set_learning_rate`` / ``set_weight_decay`` reach a captured graph's next replay without a recapture.  A float ``lr`` with no
    decay launches exactly the fixed-rate kernels it always did.  

    ``average`` (None: off - nothing is allocated, nothing new is launched, ``state_dict()`` keeps its keys) keeps an average of the weights
    along the trajectory in one more flat fp32 buffer ``avg``, initialised to the weights as tfa initialises its slot to the variable:
      * ``{"mode": "ema", "decay": 0.999, "dynamic_decay": False, "start_step": 0}``: tfa.optimizers.MovingAverage;
      * ``{"mode": "swa", "start": S, "period": P}``: tfa.optimizers.SWA - the arithmetic mean of the weights after steps S, S+P, S+2P, ...
    The update kernel of ``apply_range`` becomes the one that also blends ``avg`` (``ops.adamw_avg_step``: one more read and one more
    write per parameter, no further launch), on the table path and on the fixed-rate path alike; ``flat``, ``m`` and ``v`` get the bits they
    get without averaging.  The settings live in a device descriptor (``UssegAverage``), so ``set_average_decay`` reaches a captured
    graph's next replay.  BatchNorm moving statistics are not variables and are not averaged.

    ``accumulate`` (None or 1: off - nothing is allocated, nothing new is launched) is the number N of micro-batches whose gradients make one
    optimiser step: one more flat fp32 buffer ``acc`` holds their sum, and ``accumulate(finish)`` - a hook of
    ``step.TrainStepDriver``, like ``clip_local`` / ``apply`` - adds ``flat.grad`` to it or, on the N-th, leaves their mean in ``flat.grad`` and
    ``acc`` at zero.  Everything else here runs once per optimiser step, on that mean.
    """

    def __init__(self, flat: FlatParams, lr=1e-3, clip_norm: Optional[float] = 1.0, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=None,
                 decay_exclude: Optional[Sequence[str]] = None, average: Optional[dict] = None, accumulate: Optional[int] = None):
        self.flat, self.clip_norm = flat, clip_norm
        self.accumulate_steps = accumulate_config(accumulate)
        self.acc = torch.zeros_like(flat.grad) if self.accumulate_steps > 1 else None
        self.average = None if average is None else average_config(average)
        self.lr = _rate(lr, "lr")
        self.weight_decay = None if weight_decay is None else _rate(weight_decay, "weight_decay")
        self.b1, self.b2, self.eps = beta1, beta2, eps
        dev = flat.device
        self.m = torch.zeros_like(flat.flat)
        self.v = torch.zeros_like(flat.flat)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr_t_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sumsq = torch.zeros(ops.ACC_FLOATS, dtype=torch.float32, device=dev)   # [0] = squared global norm (reproducible accumulator)
        self.sched_dev = None            # UssegLrSchedule as int32[48] (n, boundary[15], lr bits[16], wd bits[16]); None = fixed-rate kernels
        self.wd_t_dev = None
        self.decay_mask = _decay_mask(flat, decay_exclude)
        self._captured = False
        if isinstance(self.lr, PiecewiseConstantDecay) or self.weight_decay is not None:
            self._enable_table()
        self.avg = self.avg_desc = None
        self._avg_from_weights = False       # set by a checkpoint without an average: the next ``params_loaded`` starts it from the weights
        if self.average is not None:
            self.avg = flat.flat.detach().clone()
            self.avg_desc = torch.zeros(ops.AVERAGE_WORDS, dtype=torch.int32, device=dev)
            self._write_average()

    # ---- the weight average -----------------------------------------------------------------------------------------
    def _write_average(self):
        """Stream-ordered copy of the host descriptor: a step (or graph replay) enqueued after it blends with the new settings."""
        self.avg_desc.copy_(torch.from_numpy(_average_words(self.average)))

    def set_average_decay(self, decay):
        """EMA decay from the next step on (eager or replayed)."""
        if self.average is None or self.average["mode"] != "ema":
            raise ValueError("set_average_decay: the optimiser was built without average={'mode': 'ema', ...}")
        self.average = average_config(dict(self.average, decay=decay))
        self._write_average()

    def average_state(self):
        """(mode, t, snapshots taken so far) from the device step counter and descriptor.  Synchronises: for logging."""
        if self.average is None:
            return None
        w = self.avg_desc.cpu().numpy()
        t = int(self.step_dev.item())
        mode, start, period = int(w[0]), int(w[3]), max(int(w[4]), 1)
        if mode == ops.AVERAGE_MODES["swa"]:
            return "swa", t, 0 if t < start else (t - start) // period + 1
        return "ema", t, max(t - start, 0)

    def swap_average(self):
        """Exchanges ``flat.flat`` and ``avg`` in place (one launch, no pointer changes): ``TrainStepDriver.averaged_weights`` calls it twice."""
        ops.swap_f32(self.flat.flat, self.avg)

    def params_loaded(self):
        """The model calls this after weights were written into ``flat`` from outside (``load_params``): before the first step, or after a
        checkpoint that carried no average, the average starts from those weights.  Synchronises (reads the step counter)."""
        if self.avg is not None and (self._avg_from_weights or int(self.step_dev.item()) == 0):
            self.avg.copy_(self.flat.flat)
        self._avg_from_weights = False

    # ---- the device table -------------------------------------------------------------------------------------------
    @property
    def scheduled(self) -> bool:
        """True when the step reads its rates from the device table (a schedule or a weight decay was given)."""
        return self.sched_dev is not None

    def _enable_table(self):
        if self.sched_dev is None:
            if self._captured:
                raise RuntimeError("AdamClip: a step graph captured with the fixed-rate kernels cannot follow a schedule or weight decay; "
                                   "give the schedule / weight_decay at construction, or capture the graph again after setting it")
            dev = self.flat.device
            self.sched_dev = torch.zeros(_TABLE_WORDS, dtype=torch.int32, device=dev)
            self.wd_t_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._write_table()

    def _write_table(self):
        """Stream-ordered copy of the host table: a step (or graph replay) enqueued after it reads the new rates."""
        self.sched_dev.copy_(torch.from_numpy(_table(self.lr, self.weight_decay)))

    def mark_captured(self):
        """Called by ``TrainStepDriver.capture_graph``: from now on the kernel path of the step may not change."""
        self._captured = True

    def set_learning_rate(self, lr):
        """A float or a schedule, from the next step on (eager or replayed)."""
        self.lr = _rate(lr, "lr")
        self._enable_table()

    def set_weight_decay(self, weight_decay):
        """A float or a schedule (read at the same step as the learning rate), from the next step on; 0 turns the decay off."""
        self.weight_decay = _rate(weight_decay, "weight_decay")
        self._enable_table()

    def current_learning_rate(self) -> float:
        """The (not bias-corrected) learning rate the next step uses, from the device step counter and table.  Synchronises: for logging."""
        if self.sched_dev is None:
            return float(self.lr)
        table = self.sched_dev.cpu().numpy()
        x = int(self.step_dev.item())
        n = int(table[0])
        piece = sum(1 for b in table[1:n] if x > b)
        return float(table[16:32].view(np.float32)[piece])

    # ---- the step ---------------------------------------------------------------------------------------------------
    def global_norm_sq(self):
        ops.sumsq(self.flat.grad, self.sumsq)        # sumsq[0] is overwritten: no zero-fill launch
        return self.sumsq

    def accumulate(self, finish: bool):
        """One micro-batch gradient (``flat.grad``) into ``acc``; ``finish``: the group's mean into ``flat.grad`` and ``acc`` back to zero
        (``ops.grad_accumulate``: it divides by N however many micro-steps the group really had)."""
        if self.acc is None:
            raise RuntimeError("AdamClip.accumulate: the optimiser was built without accumulate=N, N > 1")
        ops.grad_accumulate(self.acc, self.flat.grad, finish, float(self.accumulate_steps))

    def clip_local(self):
        """Per-replica clip, BEFORE the data-parallel all-reduce (VisionTransformer.py:244 precedes :245)."""
        if self.clip_norm is not None:
            self.global_norm_sq()
            ops.scale_by_clip(self.flat.grad, self.sumsq, float(self.clip_norm))

    def advance(self):
        """step += 1 and the bias-corrected learning rate of that step (device side: replayable from a HIP graph)."""
        if self.sched_dev is not None:
            ops.sched_advance(self.step_dev, self.sched_dev, self.lr_t_dev, self.wd_t_dev, self.b1, self.b2)
        else:
            ops.adam_advance(self.step_dev, self.lr_t_dev, self.lr, self.b1, self.b2)

    def apply_range(self, lo: int, hi: int, clip: float = 0.0):
        """Adam update of flat[lo:hi] (elementwise, so any partition of the buffer gives the same result as one launch)."""
        f = self.flat
        if self.avg is not None:             # the update and the average in one launch; wd_t_dev None = the fixed-rate arithmetic
            mask = None if self.decay_mask is None or self.sched_dev is None else self.decay_mask[lo:hi]
            ops.adamw_avg_step(f.flat[lo:hi], f.grad[lo:hi], self.m[lo:hi], self.v[lo:hi], self.avg[lo:hi], self.sumsq, clip, self.lr_t_dev,
                               self.wd_t_dev, mask, self.b1, self.b2, self.eps, self.step_dev, self.avg_desc)
            return
        if self.sched_dev is not None:
            mask = None if self.decay_mask is None else self.decay_mask[lo:hi]
            ops.adamw_step(f.flat[lo:hi], f.grad[lo:hi], self.m[lo:hi], self.v[lo:hi], self.sumsq, clip, self.lr_t_dev, self.wd_t_dev, mask,
                           self.b1, self.b2, self.eps)
            return
        ops.adam_clip_step(f.flat[lo:hi], f.grad[lo:hi], self.m[lo:hi], self.v[lo:hi], self.sumsq, clip, self.lr_t_dev, self.b1, self.b2,
                           self.eps)

    def apply(self, already_clipped: bool = False):
        clip = 0.0
        if self.clip_norm is not None and not already_clipped:
            # squared global norm and the step counter in one launch
            if self.sched_dev is not None:
                ops.sumsq_sched_advance(self.flat.grad, self.sumsq, self.step_dev, self.sched_dev, self.lr_t_dev, self.wd_t_dev, self.b1, self.b2)
            else:
                ops.sumsq_advance(self.flat.grad, self.sumsq, self.step_dev, self.lr_t_dev, self.lr, self.b1, self.b2)
            clip = float(self.clip_norm)
        else:
            self.advance()
        self.apply_range(0, self.flat.total, clip)

    def state_tensors(self):
        t = [self.m, self.v, self.step_dev, self.lr_t_dev]
        t = t if self.sched_dev is None else t + [self.sched_dev, self.wd_t_dev]
        t = t if self.avg is None else t + [self.avg, self.avg_desc]
        return t if self.acc is None else t + [self.acc]

    def state_dict(self):
        """Adam moments in the flat layout + the step counter (what Keras saves with a compiled model); + the rate table if one is used."""
        d = {"__adam_m__": self.m.detach().clone(), "__adam_v__": self.v.detach().clone(), "__adam_step__": self.step_dev.detach().clone()}
        if self.sched_dev is not None:
            d["__adam_sched__"] = self.sched_dev.detach().clone()
        if self.avg is not None:
            d["__adam_avg__"] = self.avg.detach().clone()
            d["__adam_avg_desc__"] = self.avg_desc.detach().clone()
        return d

    def load_state_dict(self, d):
        if not d:
            self._avg_from_weights = self.avg is not None        # a plain checkpoint: the average starts from its weights (params_loaded)
            return
        self.m.copy_(d["__adam_m__"].to(self.m.device))
        self.v.copy_(d["__adam_v__"].to(self.v.device))
        self.step_dev.copy_(d["__adam_step__"].to(self.step_dev.device))
        if "__adam_sched__" in d:           # the saved schedule / decay replace the constructor's; the step counter selects the piece
            self.lr, self.weight_decay = _from_table(d["__adam_sched__"].cpu().numpy().astype(np.int32))
            self._enable_table()
        if self.avg is not None:            # (a checkpoint's average is ignored by an optimiser built without one)
            if "__adam_avg__" in d:         # the saved settings replace the constructor's, like the rate table
                self.avg.copy_(d["__adam_avg__"].to(self.avg.device))
                self.average = _average_from_words(d["__adam_avg_desc__"].cpu().numpy().astype(np.int32))
                self._write_average()
            else:                           # no average in the checkpoint: it starts from the weights the caller loads next
                self._avg_from_weights = True
                self.avg.copy_(self.flat.flat)


# ---------------------------------------------------------------------------------------------------- table helpers
_TABLE_WORDS = C.sizeof(L.LrSchedule) // 4


def _rate(x, what):
    if isinstance(x, PiecewiseConstantDecay):
        return x
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"AdamClip: {what} must be finite, got {x}")
    return x


def _pieces(s):
    return s.boundaries if isinstance(s, PiecewiseConstantDecay) else ()


def _at(s, x) -> np.float32:
    return s(x) if isinstance(s, PiecewiseConstantDecay) else np.float32(s)


def _table(lr, wd) -> np.ndarray:
    """UssegLrSchedule of lr and wd (None: 0) over the union of their boundaries: every merged piece takes both values at a step inside it."""
    b = sorted(set(_pieces(lr)) | set(_pieces(wd)))
    if len(b) + 1 > MAX_PIECES:
        raise ValueError(f"AdamClip: learning rate and weight decay need {len(b) + 1} pieces together, at most {MAX_PIECES} are supported")
    xs = b + [b[-1] + 1] if b else [0]          # a step inside each piece: x = b[0] for x <= b[0], b[i] for b[i-1] < x <= b[i], b[-1] + 1
    t = L.LrSchedule(n=len(xs))
    t.boundary[:len(b)] = b
    t.lr[:len(xs)] = [_at(lr, x) for x in xs]
    t.wd[:len(xs)] = [0.0 if wd is None else _at(wd, x) for x in xs]
    return np.frombuffer(t, dtype=np.int32).copy()


def _from_table(t: np.ndarray):
    t = L.LrSchedule.from_buffer_copy(np.ascontiguousarray(t, dtype=np.int32))
    n = t.n
    if not 1 <= n <= MAX_PIECES:
        raise ValueError(f"AdamClip: a saved rate table with {n} pieces")
    b = t.boundary[:n - 1]
    lr, wd = np.array(t.lr[:n], dtype=np.float32), np.array(t.wd[:n], dtype=np.float32)
    mk = (lambda v: PiecewiseConstantDecay(b, v)) if n > 1 else (lambda v: float(v[0]))
    return mk(lr), mk(wd)


def _decay_mask(flat: FlatParams, exclude) -> Optional[torch.Tensor]:
    """u8 per flat element, 1 = decayed, 0 = excluded (a variable whose name matches one of the regexes); None when nothing is excluded."""
    if not exclude:
        return None
    pats = [re.compile(p) for p in ([exclude] if isinstance(exclude, str) else exclude)]
    hit = [(o, p.numel()) for n, p, o in zip(flat.names, flat.params, flat.offsets) if any(r.search(n) for r in pats)]
    if not hit:
        return None
    mask = torch.ones(flat.total, dtype=torch.uint8)
    for o, n in hit:
        mask[o:o + n] = 0
    return mask.to(flat.device)


# ---------------------------------------------------------------------------------------------------- gradient accumulation
def accumulate_config(accumulate) -> int:
    """``accumulate=`` of ``AdamClip`` and the models -> the number of micro-steps per optimiser step (None: 1); ValueError unless it is an
    integer >= 1 (a bool is not one) and at most 2^24, up to where the kernel's divisor ``(float)N`` is N itself."""
    if accumulate is None:
        return 1
    if isinstance(accumulate, bool) or not isinstance(accumulate, (int, np.integer)) or not 1 <= accumulate <= 2 ** 24:
        raise ValueError(f"accumulate must be an integer >= 1 (micro-batches per optimiser step) and <= 2^24 (the kernel divides by (float)N, "
                         f"exact up to there), got {accumulate!r}")
    return int(accumulate)


# ---------------------------------------------------------------------------------------------------- weight averaging
_EMA_KEYS = {"mode", "decay", "dynamic_decay", "start_step"}
_SWA_KEYS = {"mode", "start", "period"}


def average_config(average: dict) -> dict:
    """Validated copy of ``AdamClip(average=...)`` with every default filled in; ValueError on a bad mode, key or number."""
    if not isinstance(average, dict) or "mode" not in average:
        raise ValueError(f"average must be a dict with a 'mode' ('ema' or 'swa'), got {average!r}")
    mode = average["mode"]
    if mode not in ops.AVERAGE_MODES:
        raise ValueError(f"average: mode must be one of {tuple(ops.AVERAGE_MODES)}, got {mode!r}")
    keys = _EMA_KEYS if mode == "ema" else _SWA_KEYS
    if set(average) - keys:
        raise ValueError(f"average: unknown keys {sorted(set(average) - keys)} for mode {mode!r} (it takes {sorted(keys)})")

    def integer(name, default, lo):
        v = average.get(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v < 2 ** 31:
            raise ValueError(f"average: {name} must be an integer >= {lo}, got {v!r}")
        return int(v)
    if mode == "ema":
        decay = float(average.get("decay", 0.999))
        if not (0.0 <= decay and np.float32(decay) < 1.0):          # as the device reads it, in fp32 (NaN fails both comparisons)
            raise ValueError(f"average: decay must be in [0, 1), got {decay}")
        return {"mode": "ema", "decay": decay, "dynamic_decay": bool(average.get("dynamic_decay", False)),
                "start_step": integer("start_step", 0, 0)}
    return {"mode": "swa", "start": integer("start", 0, 0), "period": integer("period", 1, 1)}


def parse_average(text: str) -> dict:
    """The drivers' ``--average`` string: ``ema:DECAY[:dynamic]`` or ``swa:START:PERIOD`` -> the validated ``average=`` dict."""
    parts = str(text).split(":")
    try:
        if parts[0] == "ema" and len(parts) in (2, 3) and (len(parts) == 2 or parts[2] == "dynamic"):
            return average_config({"mode": "ema", "decay": float(parts[1]), "dynamic_decay": len(parts) == 3})
        if parts[0] == "swa" and len(parts) == 3:
            return average_config({"mode": "swa", "start": int(parts[1]), "period": int(parts[2])})
    except ValueError as e:
        raise ValueError(f"--average {text!r}: {e}") from None
    raise ValueError(f"--average {text!r}: expected ema:DECAY[:dynamic] or swa:START:PERIOD")


def _average_words(cfg: dict) -> np.ndarray:
    """UssegAverage as int32 words."""
    if cfg["mode"] == "ema":
        a = L.Average(L.AVERAGE_EMA, cfg["decay"], int(cfg["dynamic_decay"]), cfg["start_step"], 1)
    else:
        a = L.Average(L.AVERAGE_SWA, 0.0, 0, cfg["start"], cfg["period"])
    return np.frombuffer(a, dtype=np.int32).copy()


def _average_from_words(w: np.ndarray) -> dict:
    a = L.Average.from_buffer_copy(np.ascontiguousarray(w, dtype=np.int32))
    if a.mode == L.AVERAGE_EMA:
        return average_config({"mode": "ema", "decay": a.decay, "dynamic_decay": bool(a.dynamic_decay), "start_step": a.start})
    if a.mode == L.AVERAGE_SWA:
        return average_config({"mode": "swa", "start": a.start, "period": a.period})
    raise ValueError(f"AdamClip: a saved average descriptor with mode {a.mode}")
