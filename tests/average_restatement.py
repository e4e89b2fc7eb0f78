"""NumPy restatement of the weight-averaging rules of ``usseg_adamw_avg_step`` / ``usseg_average_update`` (include/usseg.h,
DESIGN.md section 4g-2): the blend coefficient in fp32 as the kernels execute it, the update in fp32 as executed, and an fp64 reference.

``t`` is the optimiser's step counter AFTER the increment of the step (1 for the first step), the t of Adam's bias correction.

  EMA (tfa.optimizers.MovingAverage):  t <= start -> c = 1;  else c = 1 - d_t,  d_t = decay  or  min(decay, (1+t)/(10+t))
  SWA (tfa.optimizers.SWA):            t >= start and (t-start) % period == 0 -> c = 1/(k+1), k = (t-start)/period;  else c = 0
  update:                              avg <- fma(c, p - avg, avg);  c == 0 keeps avg, c == 1 stores p
"""
import numpy as np

OFF, EMA, SWA = 0, 1, 2
F32 = np.float32


def coeff(mode, t, decay=0.0, dynamic_decay=False, start=0, period=1) -> np.float32:
    """The fp32 blend coefficient of step ``t``: every operation below is a single correctly rounded fp32 operation, as on the device."""
    t = int(t)
    if mode == EMA:
        if t <= start:
            return F32(1.0)
        d = F32(decay)
        if dynamic_decay:
            d = min(d, F32(1 + t) / F32(10 + t))
        return F32(1.0) - d
    if mode == SWA:
        period = max(int(period), 1)
        if t < start or (t - start) % period != 0:
            return F32(0.0)
        return F32(1.0) / F32((t - start) // period + 1)
    return F32(0.0)


def update64(avg, p, c) -> np.ndarray:
    """fp64 reference of one update from fp32 inputs: avg + c*(p - avg) with the fp32 coefficient ``c`` taken exactly."""
    avg, p = np.asarray(avg, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if c == 0:
        return avg.copy()
    if c == 1:
        return p.copy()
    return avg + np.float64(c) * (p - avg)


def update32(avg, p, c) -> np.ndarray:
    """The update as executed: one fp32 rounding of the difference, then the fused multiply-add (its exact product and sum formed in fp64 -
    the 48-bit product is exact there - and rounded to fp32; the intermediate fp64 rounding can differ from a true fma in rare ties)."""
    avg, p = np.asarray(avg, dtype=F32), np.asarray(p, dtype=F32)
    if c == 0:
        return avg.copy()
    if c == 1:
        return p.copy()
    d = (p - avg).astype(F32)
    return (np.float64(c) * d.astype(np.float64) + avg.astype(np.float64)).astype(F32)


def bound(avg_old, p) -> np.ndarray:
    """|device - update64| per element: one rounding of the difference plus one of the fma, 2^-24 * (|p| + |avg|) each at most."""
    return 2.0 ** -23 * (np.abs(np.asarray(p, dtype=np.float64)) + np.abs(np.asarray(avg_old, dtype=np.float64)))


def snapshots_so_far(mode, t, start=0, period=1) -> int:
    if mode == SWA:
        return 0 if t < start else (t - start) // max(int(period), 1) + 1
    return max(t - start, 0)
