"""Test helpers for the conv route matrix: which device kernels a call launched, and a per-element error bound.

kernels(fn) runs fn under torch.profiler (device activity only) and returns (fn's result, the demangled names of the
device kernels it launched, in launch order).  A call that records no device kernel fails the test: a probe that cannot
see the launches must never turn into a pass or a skip.

assert_elementwise(y, ref, mag, u, c) checks |y - ref| <= c * u * mag + tiny for every element, in fp64, where mag is
the same operation applied to |x| and |w| (so it bounds every partial sum the kernel formed).  The relative-L2 checks
of test_gpu_ops.py average an error over the whole tensor; this one fails on a single wrong element.
"""
import pytest
import torch

U_BF16 = 2.0 ** -8      # unit roundoff of a bf16 output (one final rounding)
U_F32 = 2.0 ** -20      # fp32 outputs: 2^-24 per rounding, x16 margin; the callers scale c with the sum length K
C_BOUND = 4.0           # stated constant for bf16 outputs (one final rounding of 2^-9 dominates the fp32 sum's error);
                        # fp32 outputs use c = 4 + sqrt(K)/8 - a chosen constant that follows the random-walk growth of a K-term
                        # fp32 sum, not a proven worst case (which grows like K)
TINY = 1e-6


def kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name for e in evs if not e.name.startswith(("Memcpy", "Memset", "memcpy", "memset"))]
    if not names:
        pytest.fail("the profiler recorded no device kernel for this call: the route cannot be checked")
    return out, names


def short(name):
    """'void conv_halo_persist_kernel<2>(HaloMulti, int)' -> 'conv_halo_persist_kernel<2>'."""
    n = name
    if n.startswith("void "):
        n = n[5:]
    depth = 0
    for i, ch in enumerate(n):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return n[:i].strip()
    return n.strip()


def routed(fn, *expected):
    """Run fn, assert every name in `expected` is a launched kernel (exact short name, or a prefix ending in '<' or
    the bare kernel name), and return fn's result and the short names."""
    out, names = kernels(fn)
    got = [short(n) for n in names]
    for e in expected:
        if not any(g == e or (e.endswith("<") and g.startswith(e)) or g.split("<")[0] == e for g in got):
            pytest.fail(f"expected kernel {e!r}, launched {got}")
    return out, got


def assert_elementwise(y, ref, mag, u, c=C_BOUND, tiny=TINY, what=""):
    y = y.detach().double().cpu()
    ref = ref.detach().double().cpu()
    mag = mag.detach().double().cpu()
    assert y.shape == ref.shape == mag.shape, (y.shape, ref.shape, mag.shape)
    err = (y - ref).abs()
    lim = c * u * mag + tiny
    bad = err > lim
    if bad.any():
        idx = bad.nonzero()
        first = tuple(idx[0].tolist())
        ratio = (err / lim).max().item()
        pytest.fail(f"{what}: {int(bad.sum())} of {y.numel()} elements exceed c*u*(|x|*|w|)+tiny "
                    f"(worst ratio {ratio:.2f}); first at {first}: got {y[first].item():.6g}, ref {ref[first].item():.6g}, "
                    f"bound {lim[first].item():.3g}")
