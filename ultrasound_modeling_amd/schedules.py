"""Learning-rate / weight-decay schedules that the optimiser evaluates on the device.

``PiecewiseConstantDecay(boundaries, values)`` is ``tf.keras.optimizers.schedules.PiecewiseConstantDecay`` as the reference builds
it (MainNumpy.py:83-88, MainParallel.py:74-79).  Called on the host it returns the float32 value of step ``x``; ``flat.AdamClip``
turns it into the device table ``UssegLrSchedule`` (include/usseg.h) that the step kernels read at the device step counter, so a
captured graph follows it.  ``c * schedule`` is the schedule of the products ``fl32(fl32(c) * fl32(v))``: the bits TensorFlow computes
for ``1e-2 * schedule(iteration)``.
"""
from __future__ import annotations

import math
import numbers
from typing import Sequence

import numpy as np

from ._lib import SCHED_MAX_PIECES as MAX_PIECES

_I32_MAX = 2 ** 31 - 1


class PiecewiseConstantDecay:
    """x <= b[0] -> v[0];  b[i-1] < x <= b[i] -> v[i];  x > b[-1] -> v[-1]  (Keras' rule).  ``len(values) == len(boundaries) + 1``,
    boundaries strictly increasing integers in [0, 2^31 - 1), at most 16 pieces, finite values."""

    def __init__(self, boundaries: Sequence[int], values: Sequence[float]):
        b = list(boundaries)
        v = list(values)
        if len(v) != len(b) + 1:
            raise ValueError(f"PiecewiseConstantDecay: {len(v)} values for {len(b)} boundaries (need len(boundaries) + 1)")
        if len(v) > MAX_PIECES:
            raise ValueError(f"PiecewiseConstantDecay: {len(v)} pieces, at most {MAX_PIECES} are supported")
        for x in b:
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise TypeError(f"PiecewiseConstantDecay: boundary {x!r} is not an integer step")
            if not 0 <= int(x) < _I32_MAX:
                raise ValueError(f"PiecewiseConstantDecay: boundary {x} outside [0, 2^31 - 1)")
        if any(int(b[i]) >= int(b[i + 1]) for i in range(len(b) - 1)):
            raise ValueError(f"PiecewiseConstantDecay: boundaries {b} are not strictly increasing")
        for x in v:
            if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(float(x)):
                raise ValueError(f"PiecewiseConstantDecay: value {x!r} is not a finite number")
        self.boundaries = tuple(int(x) for x in b)
        self.values = np.asarray(v, dtype=np.float32)          # Keras converts the values to float32 tensors

    def piece(self, x: int) -> int:
        """Index of the value step ``x`` uses: the number of boundaries strictly below x."""
        return sum(1 for b in self.boundaries if x > b)

    def __call__(self, x) -> np.float32:
        return self.values[self.piece(int(x))]

    def __mul__(self, c):
        if isinstance(c, bool) or not isinstance(c, numbers.Real):
            return NotImplemented
        out = PiecewiseConstantDecay.__new__(PiecewiseConstantDecay)
        out.boundaries = self.boundaries
        out.values = (np.float32(c) * self.values).astype(np.float32)     # one float32 rounding per piece
        return out

    __rmul__ = __mul__

    def __eq__(self, other):
        return (isinstance(other, PiecewiseConstantDecay) and self.boundaries == other.boundaries
                and self.values.tobytes() == other.values.tobytes())

    def __repr__(self):
        return f"PiecewiseConstantDecay({list(self.boundaries)}, {[float(v) for v in self.values]})"
