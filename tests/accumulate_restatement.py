"""NumPy fp32 restatement of ``usseg_grad_accumulate`` (include/usseg_accumulate.h) and of a group of N micro-steps.

  micro-step   (finish == 0):  acc <- acc + grad
  finishing    (finish == 1):  t = acc + grad;  grad <- t / N;  acc <- 0

Every operation is one correctly rounded IEEE fp32 operation on the device (an add, a true division), which is what NumPy does on float32
arrays - so the restatement is exact for every N, 3 included, for -0.0, denormals, infinities and (up to the payload, which IEEE 754 leaves
open) NaNs.
"""
import numpy as np

F32 = np.float32


def micro(acc, grad) -> np.ndarray:
    """-> the new accumulator; ``grad`` is left as it is."""
    acc, grad = np.asarray(acc, dtype=F32), np.asarray(grad, dtype=F32)
    with np.errstate(all="ignore"):
        return (acc + grad).astype(F32)


def finish(acc, grad, n):
    """-> (the new accumulator: all +0.0, the finished gradient)."""
    acc, grad = np.asarray(acc, dtype=F32), np.asarray(grad, dtype=F32)
    with np.errstate(all="ignore"):
        t = (acc + grad).astype(F32)
        return np.zeros_like(acc), (t / F32(n)).astype(F32)


def group(grads, n):
    """The gradient the optimiser sees after the micro-batch gradients ``grads`` (k <= n of them, in order) of a group of ``n``: k - 1
    micro-steps from a zero accumulator and one finishing step.  k < n is ``flush_step()`` - it still divides by n - and gives the bits of
    a full group whose remaining gradients are +0.0."""
    grads = [np.asarray(g, dtype=F32) for g in grads]
    assert 1 <= len(grads) <= n
    acc = np.zeros_like(grads[0])
    for g in grads[:-1]:
        acc = micro(acc, g)
    return finish(acc, grads[-1], n)[1]


def same_bits(got, want) -> np.ndarray:
    """Per element: the same 32 bits, or both NaN (IEEE 754 does not fix which NaN an operation on a NaN returns)."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
