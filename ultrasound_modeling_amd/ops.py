"""Thin torch-tensor front end of the C ABI (include/usseg.h).

torch is used for device memory and the current HIP stream only; every function here enqueues
hand-written gfx950 kernels from libusseg_hip.so and raises if the library is missing.

Activation tensors are bf16 ``[B,H,W,Cphys]`` (NHWC) or channel-slice views of such tensors
(``t[..., a:b]`` with a, b multiples of 8); the channel stride ``ld`` is taken from the view.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import knobs
from ._lib import (ACCUMULATE, ACT_ELU, ACT_GELU, ACT_LRELU, ACT_NONE, ACT_RELU, OUT_F32, CardinalDesc, ConvDesc, GemmDesc, LossDesc, NormDesc,
                   SplitAttnDesc, SplitAttnGrads, SplitAttnParams)

BF16 = torch.bfloat16
ACC_FLOATS = L.ACC_FLOATS   # a reproducible scalar accumulator ([0] result, [1] ticket, [2..] per-workgroup partials)


def roundup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_REDUCE_WS = {}
_WGRAD_WS = {}
WGRAD_WS_FLOATS = 64 << 20   # 256 MB of the 288 GB: split-K partial slabs of the 3x3 weight-gradient kernel


# ------------------------------------------------------------------------------------------------ side stream
# Weight gradients never feed the backward-data chain, so inside an ``overlap_region`` (the model's backward pass) they
# are enqueued on a second HIP stream and run beside the dgrad / norm-backward kernels of the main stream (which leave
# most CUs under-occupied at batch 16).  Both streams are captured into the same HIP graph (fork by event, join at the
# end of the region).  Workspaces are per stream; the tensors a side launch reads are kept alive until the join so the
# caching allocator cannot hand their memory to a later main-stream tensor.
# Off by default since the conv / wgrad kernels got ~1.5x faster: the fork/join edges of the captured graph now cost more
# than the overlap returns (Arch B 4.17 vs 4.23 ms, Arch A 9.47 vs 9.87 ms per step; USSEG_SIDE_STREAM=1 turns it back on).
# The fork needs a hardware queue of its own for the side stream: with GPU_MAX_HW_QUEUES below 3 (the runtime's default is 4) the
# replay of a captured two-stream step crashes or never finishes, so there nothing forks and the side-stream launches run in line on
# the current stream, in the order they were queued (the same bits: tests/test_gpu_concurrency.py).
def _fork_allowed(max_hw_queues: Optional[str]) -> bool:
    """Whether the side stream may fork, given the value of GPU_MAX_HW_QUEUES (None: unset, the runtime's default of 4).  Any value
    below 3 - 0 included - means no fork; a value that is not a number is taken as the default."""
    try:
        n = int(max_hw_queues) if max_hw_queues else 4
    except ValueError:
        n = 4
    return n >= 3


class _Side:
    # read once, like the HIP runtime itself, which takes the setting when it loads (with torch, before this module)
    fork = _fork_allowed(os.environ.get("GPU_MAX_HW_QUEUES"))
    enabled = knobs.get("USSEG_SIDE_STREAM")
    defer = knobs.get("USSEG_DEFER")
    depth = 0
    stream = None
    keep = []
    dirty = False
    deferring = set()      # stream handles with an open deferral context
    post = []              # callbacks that run after the region's final flush (ops.after_flush)
    bufs = {}


DEFER_REDUCE_FLOATS = 32 << 20    # 128 MB of partial rows per stream
DEFER_WGRAD_FLOATS = 256 << 20    # 1 GB of split-K slabs per stream (of 288 GB): the whole backward pass between flushes


def _defer_begin():
    """Queue the finishing reductions of the current stream (usseg_defer_begin) until _defer_end."""
    if not _Side.defer:
        return
    h = _stream()
    if h in _Side.deferring:
        return
    dev = torch.cuda.current_device()
    key = (dev, torch.cuda.current_stream() == _Side.stream)
    if key not in _Side.bufs:
        _Side.bufs[key] = (torch.empty(DEFER_REDUCE_FLOATS, dtype=torch.float32, device="cuda"),
                           torch.empty(DEFER_WGRAD_FLOATS, dtype=torch.float32, device="cuda"))
    r, w = _Side.bufs[key]
    L.check(L.load().usseg_defer_begin(h, r.data_ptr(), r.numel(), w.data_ptr(), w.numel()), "defer_begin")
    _Side.deferring.add(h)


def _defer_end():
    h = _stream()
    if h in _Side.deferring:
        _Side.deferring.discard(h)
        L.check(L.load().usseg_defer_end(h), "defer_end")


def defer_flush():
    """Run the queued finishing reductions of the current stream now (their gradients are about to be read)."""
    if _stream() in _Side.deferring:
        L.check(L.load().usseg_defer_flush(_stream()), "defer_flush")


def after_flush(fn):
    """Run ``fn`` once the finishing reductions queued so far have executed: at the end of the enclosing ``overlap_region``
    (after its final flush - no extra finishing launches in the middle of the backward pass), or right away when nothing is
    being deferred."""
    if _Side.depth > 0 and _stream() in _Side.deferring and not (_Side.enabled and _Side.stream is not None and torch.cuda.current_stream() == _Side.stream):
        _Side.post.append(fn)
    else:
        defer_flush()
        fn()


@contextlib.contextmanager
def overlap_region():
    _Side.depth += 1
    if _Side.depth == 1:
        _defer_begin()
    try:
        yield
    finally:
        _Side.depth -= 1
        if _Side.depth == 0:
            side_join()
            _defer_end()
            post, _Side.post = _Side.post, []
            for fn in post:
                fn()


@contextlib.contextmanager
def side_stream(*keep):
    """Enqueue the enclosed launches on the side stream, ordered after everything already on the current stream."""
    if not (_Side.enabled and _Side.fork and _Side.depth > 0):
        yield
        return
    if _Side.stream is None:
        _Side.stream = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(main)
    _Side.stream.wait_event(ev)
    _Side.keep.extend(keep)
    _Side.dirty = True
    with torch.cuda.stream(_Side.stream):
        _defer_begin()
        yield


# Lazy weight gradients (USSEG_LAZY_WGRAD, default on): inside ``lazy_wgrads()`` the weight-gradient launches handed to
# ``wgrad_later`` are only collected; at the end of the block they all run on the side stream behind ONE fork, beside whatever the
# main stream does next (the encoder's backward pass), and join at the end of the overlap region.  The per-layer fork of
# ``side_stream`` (USSEG_SIDE_STREAM=1) costs a cross-stream edge per launch, which made it slower than a single stream.
_LAZY = knobs.get("USSEG_LAZY_WGRAD")
_lazy_q = None


@contextlib.contextmanager
def lazy_wgrads():
    global _lazy_q
    if not _LAZY or _Side.depth == 0 or _lazy_q is not None:
        yield
        return
    _lazy_q = []
    try:
        yield
    finally:
        q, _lazy_q = _lazy_q, None
        if q:
            enabled, _Side.enabled = _Side.enabled, True
            try:
                with side_stream(*[t for _, keep in q for t in keep]):
                    for fn, _ in q:
                        fn()
            finally:
                _Side.enabled = enabled


def wgrad_later(fn, *keep):
    """Run ``fn`` (weight-gradient launches reading the tensors ``keep``) now - on the side stream if that is enabled - or, inside
    ``lazy_wgrads()``, at the end of that block."""
    if _lazy_q is not None:
        _lazy_q.append((fn, keep))
        return
    with side_stream(*keep):
        fn()


def side_join():
    if _Side.dirty:
        with torch.cuda.stream(_Side.stream):
            _defer_end()
        ev = torch.cuda.Event()
        ev.record(_Side.stream)
        torch.cuda.current_stream().wait_event(ev)
        _Side.dirty = False
    _Side.keep.clear()


def _ws_key(device):
    on_side = _Side.stream is not None and torch.cuda.current_stream() == _Side.stream
    return (str(device), on_side)


def wgrad_ws(device) -> torch.Tensor:
    key = _ws_key(device)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = torch.empty(WGRAD_WS_FLOATS, dtype=torch.float32, device=device)
        _WGRAD_WS[key] = ws
    return ws



def reduce_ws(device) -> torch.Tensor:
    """fp32 workspace for the library's two-pass per-channel reductions (one per device and stream; stream order serialises its users)."""
    key = _ws_key(device)
    ws = _REDUCE_WS.get(key)
    if ws is None:
        ws = torch.empty(int(L.load().usseg_reduce_ws_floats()), dtype=torch.float32, device=device)
        _REDUCE_WS[key] = ws
    return ws


def geom(t: torch.Tensor) -> Tuple[int, int, int, int, int]:
    """(B,H,W,C,ld) of an NHWC tensor or channel-slice view; validates the layout."""
    assert t.dim() == 4, f"expected NHWC tensor, got shape {tuple(t.shape)}"
    B, H, W, Cc = t.shape
    assert t.stride(3) == 1 or Cc == 1, "channels must be contiguous"
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else Cc))
    if W > 1 and H > 1:
        assert t.stride(1) == W * ld, "rows must be dense"
    if B > 1:
        assert t.stride(0) == H * W * ld, "images must be dense"
    return B, H, W, Cc, ld


def new_act(B: int, H: int, W: int, Cphys: int, device, zero: bool = False) -> torch.Tensor:
    f = torch.zeros if zero else torch.empty
    return f((B, H, W, Cphys), dtype=BF16, device=device)


def _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation=1, act=ACT_NONE, alpha=0.0, flags=0) -> ConvDesc:
    return ConvDesc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation, act, alpha, flags)


# ------------------------------------------------------------------------------------------------ conv
def conv2d_fwd(x, wp, bias, ksize, dilation, out, act=ACT_NONE, alpha=0.0, residual=None, out_f32=False, scale=None):
    """``scale`` (fp32 per output channel): y = act(scale*conv + bias) - the folded inference BatchNorm (bias = its shift)."""
    B, H, W, Cin, ldx = geom(x)
    Bo, Ho, Wo, Cout, ldy = geom(out)
    assert (Bo, Ho, Wo) == (B, H, W)
    assert x.dtype == BF16 and out.dtype == (torch.float32 if out_f32 else BF16)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation, act, alpha, OUT_F32 if out_f32 else 0)
    ldr = geom(residual)[4] if residual is not None else 0
    if scale is not None:
        L.check(L.load().usseg_conv2d_fwd_affine(C.byref(d), x.data_ptr(), wp.data_ptr(), scale.data_ptr(), bias.data_ptr(), _ptr(residual),
                                                 ldr, out.data_ptr(), _stream()), "conv2d_fwd_affine")
        return out
    L.check(L.load().usseg_conv2d_fwd(C.byref(d), x.data_ptr(), wp.data_ptr(), _ptr(bias), _ptr(residual), ldr,
                                      out.data_ptr(), _stream()), "conv2d_fwd")
    return out


def conv2d_dgrad(dy, wp_d, ksize, dilation, dx, residual=None, accumulate=False):
    B, H, W, Cout, ldy = geom(dy)
    _, _, _, Cin, ldx = geom(dx)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation, flags=ACCUMULATE if accumulate else 0)
    ldr = geom(residual)[4] if residual is not None else 0
    L.check(L.load().usseg_conv2d_dgrad(C.byref(d), dy.data_ptr(), wp_d.data_ptr(), _ptr(residual), ldr, dx.data_ptr(),
                                        _stream()), "conv2d_dgrad")
    return dx


def conv2d_fwd_multi(jobs):
    """jobs: list of (x, wp, bias, ksize, dilation, out, act, alpha) of INDEPENDENT convs -> one launch where possible."""
    arr = (L.ConvJob * len(jobs))()
    for j, job in enumerate(jobs):
        x, wp, bias, ksize, dilation, out, act, alpha = job[:8]
        arr[j].scale = _ptr(job[8]) if len(job) > 8 else None      # optional folded-BatchNorm multiplier (bias = its shift)
        B, H, W, Cin, ldx = geom(x)
        Bo, Ho, Wo, Cout, ldy = geom(out)
        assert (Bo, Ho, Wo) == (B, H, W) and x.dtype == BF16 and out.dtype == BF16
        arr[j].desc = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation, act, alpha, 0)
        arr[j].x, arr[j].wp, arr[j].bias, arr[j].residual, arr[j].ldr, arr[j].y = x.data_ptr(), wp.data_ptr(), _ptr(bias), None, 0, out.data_ptr()
    L.check(L.load().usseg_conv2d_fwd_multi(len(jobs), arr, _stream()), "conv2d_fwd_multi")


def conv2d_dgrad_multi(jobs):
    """jobs: list of (dy, wp_d, ksize, dilation, dx, residual, accumulate) writing DISJOINT dx buffers -> one launch where possible."""
    arr = (L.ConvJob * len(jobs))()
    for j, (dy, wp_d, ksize, dilation, dx, residual, accumulate) in enumerate(jobs):
        B, H, W, Cout, ldy = geom(dy)
        _, _, _, Cin, ldx = geom(dx)
        arr[j].desc = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation, flags=ACCUMULATE if accumulate else 0)
        arr[j].x, arr[j].wp, arr[j].bias, arr[j].y = dy.data_ptr(), wp_d.data_ptr(), None, dx.data_ptr()
        arr[j].residual, arr[j].ldr = _ptr(residual), (geom(residual)[4] if residual is not None else 0)
    L.check(L.load().usseg_conv2d_dgrad_multi(len(jobs), arr, _stream()), "conv2d_dgrad_multi")


def conv2d_wgrad(x, dy, ksize, dilation, dw: torch.Tensor):
    """dw (fp32, [ntaps, Cin_phys, Cout_phys], pre-zeroed or holding a running sum) += x^T dy."""
    B, H, W, Cin, ldx = geom(x)
    _, _, _, Cout, ldy = geom(dy)
    assert dw.dtype == torch.float32 and dw.numel() == ksize * ksize * Cin * Cout
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation)
    ws = wgrad_ws(x.device)
    L.check(L.load().usseg_conv2d_wgrad(C.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "conv2d_wgrad")
    return dw


def wgrad_dst(blocks) -> "L.WgradDst":
    """blocks: list of (dst tensor, sT, sI, sO, i_off, o_off, ni, no) -> destination map of a mapped weight gradient."""
    m = L.WgradDst()
    m.nblocks = len(blocks)
    for b, (dst, sT, sI, sO, i_off, o_off, ni, no) in enumerate(blocks):
        assert dst.dtype == torch.float32
        m.blk[b].dst, m.blk[b].sT, m.blk[b].sI, m.blk[b].sO = dst.data_ptr(), sT, sI, sO
        m.blk[b].i_off, m.blk[b].o_off, m.blk[b].ni, m.blk[b].no = i_off, o_off, ni, no
    return m


def conv2d_wgrad_mapped(x, dy, ksize, dilation, dst_map):
    """dW (physical [ntaps][Cin_phys][Cout_phys]) accumulated straight into the variables named by ``dst_map`` (no scratch pass)."""
    B, H, W, Cin, ldx = geom(x)
    _, _, _, Cout, ldy = geom(dy)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation)
    ws = wgrad_ws(x.device)
    L.check(L.load().usseg_conv2d_wgrad_mapped(C.byref(d), x.data_ptr(), dy.data_ptr(), C.byref(dst_map), ws.data_ptr(), ws.numel(),
                                               _stream()), "conv2d_wgrad_mapped")


def conv2d_dgrad_branches(dy_cat, wp_cat, ksizes, dilations, ch_offs, Cb, dx, residual=None, accumulate=False):
    """dx = sum over the parallel branches of their backward-data passes (one implicit GEMM over every branch's taps)."""
    B, H, W, _, ldy = geom(dy_cat)
    _, _, _, Cin, ldx = geom(dx)
    d = _conv_desc(B, H, W, Cin, Cb, ldx, ldy, 3, 1, flags=ACCUMULATE if accumulate else 0)
    n = len(ksizes)
    arr = lambda v: (C.c_int32 * n)(*v)
    ldr = geom(residual)[4] if residual is not None else 0
    L.check(L.load().usseg_conv2d_dgrad_branches(C.byref(d), n, arr(ksizes), arr(dilations), arr(ch_offs), Cb, dy_cat.data_ptr(),
                                                 wp_cat.data_ptr(), _ptr(residual), ldr, dx.data_ptr(), _stream()), "conv2d_dgrad_branches")
    return dx


def conv2d_wgrad_multi(jobs):
    """jobs: list of (x, dy, ksize, dilation, dw or None, dst_map or None): independent weight gradients, one launch where possible."""
    arr = (L.WgradJob * len(jobs))()
    for j, (x, dy, ksize, dilation, dw, dst_map) in enumerate(jobs):
        B, H, W, Cin, ldx = geom(x)
        _, _, _, Cout, ldy = geom(dy)
        arr[j].desc = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, dilation)
        arr[j].x, arr[j].dy, arr[j].dw = x.data_ptr(), dy.data_ptr(), _ptr(dw)
        arr[j].dst = C.pointer(dst_map) if dst_map is not None else None
    ws = wgrad_ws(jobs[0][0].device)
    L.check(L.load().usseg_conv2d_wgrad_multi(len(jobs), arr, ws.data_ptr(), ws.numel(), _stream()), "conv2d_wgrad_multi")


def tconv2d_wgrad_mapped(x, dy, ksize, dst_map):
    B, H, W, Cin, ldx = geom(x)
    _, _, _, Cout, ldy = geom(dy)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, 1)
    ws = wgrad_ws(x.device)
    L.check(L.load().usseg_tconv2d_wgrad_mapped(C.byref(d), x.data_ptr(), dy.data_ptr(), C.byref(dst_map), ws.data_ptr(), ws.numel(),
                                                _stream()), "tconv2d_wgrad_mapped")


def tconv2d_fwd(x, wp, bias, ksize, out, act=ACT_NONE, alpha=0.0, out_f32=False):
    B, H, W, Cin, ldx = geom(x)
    Bo, Ho, Wo, Cout, ldy = geom(out)
    assert (Bo, Ho, Wo) == (B, 2 * H, 2 * W)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, 1, act, alpha, OUT_F32 if out_f32 else 0)
    L.check(L.load().usseg_tconv2d_fwd(C.byref(d), x.data_ptr(), wp.data_ptr(), _ptr(bias), out.data_ptr(), _stream()),
            "tconv2d_fwd")
    return out


def tconv2d_dgrad(dy, wp_d, ksize, dx, residual=None, accumulate=False):
    B, H2, W2, Cout, ldy = geom(dy)
    Bx, H, W, Cin, ldx = geom(dx)
    assert (H2, W2) == (2 * H, 2 * W)
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, 1, flags=ACCUMULATE if accumulate else 0)
    ldr = geom(residual)[4] if residual is not None else 0
    L.check(L.load().usseg_tconv2d_dgrad(C.byref(d), dy.data_ptr(), wp_d.data_ptr(), _ptr(residual), ldr, dx.data_ptr(),
                                         _stream()), "tconv2d_dgrad")
    return dx


def tconv2d_wgrad(x, dy, ksize, dw: torch.Tensor):
    """dw (fp32, [ntaps, Cin_phys, Cout_phys]) += sum_i x[i] (x) dy[2i+k-pad]."""
    B, H, W, Cin, ldx = geom(x)
    _, _, _, Cout, ldy = geom(dy)
    assert dw.dtype == torch.float32 and dw.numel() == ksize * ksize * Cin * Cout
    d = _conv_desc(B, H, W, Cin, Cout, ldx, ldy, ksize, 1)
    L.check(L.load().usseg_tconv2d_wgrad(C.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _stream()), "tconv2d_wgrad")
    return dw


def pack_weight(src: torch.Tensor, sT, sN, sK, T, Nn, Kk, dst: torch.Tensor, Kw, tap_stride, n_off=0, k_off=0):
    assert src.dtype == torch.float32 and dst.dtype == BF16
    L.check(L.load().usseg_pack_weight(src.data_ptr(), sT, sN, sK, T, Nn, Kk, dst.data_ptr(), Kw, tap_stride, n_off, k_off,
                                       _stream()), "pack_weight")


PACK_JOB_DTYPE = np.dtype(L.PackJob)


def pack_job(src, sT, sN, sK, T, Nn, Kk, dst, Kw, tap_stride, n_off=0, k_off=0, nscale=None):
    """Descriptor tuple of one pack (same arguments as pack_weight) for pack_weights_batched.  ``nscale``: optional fp32 vector,
    one multiplier per row n (an inference BatchNorm folded into the forward operand)."""
    assert src.dtype == torch.float32 and dst.dtype == BF16
    assert nscale is None or (nscale.dtype == torch.float32 and nscale.numel() >= Nn)
    return (src.data_ptr(), dst.data_ptr(), sT, sN, sK, T, Nn, Kk, Kw, tap_stride, n_off, k_off, 0, 0 if nscale is None else nscale.data_ptr())


def make_pack_table(jobs, device) -> torch.Tensor:
    arr = np.array(jobs, dtype=PACK_JOB_DTYPE)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


BN_FOLD_JOB_DTYPE = np.dtype(L.BnFoldJob)


def bn_fold_job(gamma, beta, mean, var, bias, scale, shift, C_logical, eps):
    """Descriptor of one folded inference BatchNorm: scale = gamma*rsqrt(var+eps), shift = beta - mean*scale + scale*bias."""
    return (gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), bias.data_ptr() if bias is not None else 0,
            scale.data_ptr(), shift.data_ptr(), C_logical, scale.numel(), eps, 0)


def make_bn_fold_table(jobs, device) -> torch.Tensor:
    arr = np.array(jobs, dtype=BN_FOLD_JOB_DTYPE)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def bn_fold_batched(table: torch.Tensor, njobs: int):
    L.check(L.load().usseg_bn_fold_batched(table.data_ptr(), njobs, _stream()), "bn_fold_batched")


def make_pack_tilemap(jobs, device, tiles_per_block: int = 4):
    """(job, first tile, count) triples covering every 32x32 tile of every pack job once -> (int32 device tensor, nblocks)."""
    trip = []
    for ji, job in enumerate(jobs):
        T, Nn, Kk = job[5], job[6], job[7]
        n = T * ((Nn + 31) // 32) * ((Kk + 31) // 32)
        for t0 in range(0, n, tiles_per_block):
            trip.append((ji, t0, min(tiles_per_block, n - t0)))
    arr = np.array(trip, dtype=np.int32).reshape(-1)
    return torch.from_numpy(arr).to(device), len(trip)


def pack_weights_batched(table: torch.Tensor, njobs: int, tilemap=None):
    if tilemap is not None:
        L.check(L.load().usseg_pack_weights_flat(table.data_ptr(), tilemap[0].data_ptr(), tilemap[1], _stream()), "pack_weights_flat")
        return
    L.check(L.load().usseg_pack_weights_batched(table.data_ptr(), njobs, _stream()), "pack_weights_batched")


def unpack_wgrad(scratch, Mrows, Ncols, T, Nn, Kk, n_off, k_off, dst, sT, sN, sK, scale=1.0, accumulate=True):
    L.check(L.load().usseg_unpack_wgrad(scratch.data_ptr(), Mrows, Ncols, T, Nn, Kk, n_off, k_off, dst.data_ptr(), sT, sN, sK,
                                        scale, 1 if accumulate else 0, _stream()), "unpack_wgrad")


UNPACK_JOB_DTYPE = np.dtype(L.UnpackJob)


def unpack_job(scratch, Mrows, Ncols, T, Nn, Kk, n_off, k_off, dst, sT, sN, sK, scale=1.0, accumulate=True):
    return (scratch.data_ptr(), dst.data_ptr(), sT, sN, sK, Mrows, Ncols, T, Nn, Kk, n_off, k_off, 1 if accumulate else 0, scale, 0)


def make_unpack_table(jobs, device):
    arr = np.array(jobs, dtype=UNPACK_JOB_DTYPE)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(jobs), int(max(j[7] * j[8] * j[9] for j in jobs))


def unpack_wgrad_batched(table):
    t, n, mx = table
    L.check(L.load().usseg_unpack_wgrad_batched(t.data_ptr(), n, mx, _stream()), "unpack_wgrad_batched")


# ------------------------------------------------------------------------------------------------ norm / act / pool
def _norm_desc(x, C_logical, out_ld, G, mode, eps, act, alpha) -> NormDesc:
    B, H, W, Cphys, ldx = geom(x)
    return NormDesc(B * H * W, C_logical, Cphys, ldx, out_ld, G, mode, eps, act, alpha)


def _readable(t: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    """The norm kernels read their per-channel vectors in 16-byte pieces up to Cphys floats (include/usseg.h).  The model's vectors
    are views of the flat parameter buffer, where every variable is padded to 8 floats; a stand-alone C-float tensor (tests) is
    copied into a padded one so the kernel never reads past an allocation."""
    if t is None or t.numel() >= n or t.storage_offset() + n <= t.untyped_storage().nbytes() // t.element_size():
        return t
    out = torch.zeros(n, dtype=t.dtype, device=t.device)
    out[:t.numel()] = t.reshape(-1)
    return out


def norm_act_fwd(x, C_logical, gamma, beta, out, mode, G=1, eps=1e-3, act=ACT_NONE, alpha=0.0, mean=None, var=None, mask=None):
    d = _norm_desc(x, C_logical, geom(out)[4], G, mode, eps, act, alpha)
    gamma, beta, mean, var = (_readable(t, d.Cphys) for t in (gamma, beta, mean, var))
    ldm = geom(mask)[4] if mask is not None else 0
    L.check(L.load().usseg_norm_act_fwd(C.byref(d), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(mean), _ptr(var),
                                        _ptr(mask), ldm, out.data_ptr(), _stream()), "norm_act_fwd")
    return out


def norm_act_fwd_gap(x, C_logical, gamma, beta, out, mode, G=1, eps=1e-3, act=ACT_NONE, alpha=0.0, mean=None, var=None):
    """norm + activation that also emits the partial rows of the global average pool of its output (split attention,
    ResNest.py:179): -> (out, (rows [B,nb,Cphys] fp32, nb, Cphys)) for ``splitattn_fwd(..., gap=...)``."""
    B, H, W, Cphys, _ = geom(x)
    d = _norm_desc(x, C_logical, geom(out)[4], G, mode, eps, act, alpha)
    gamma, beta, mean, var = (_readable(t, Cphys) for t in (gamma, beta, mean, var))
    nb = max(1, min(32, (H * W) // 32))
    rows = torch.empty((B, nb, Cphys), dtype=torch.float32, device=x.device)
    L.check(L.load().usseg_norm_act_fwd_gap(C.byref(d), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(mean), _ptr(var), out.data_ptr(),
                                            B, nb, rows.data_ptr(), _stream()), "norm_act_fwd_gap")
    return out, (rows, nb, Cphys)


def norm_act_bwd_sa(x, dout, C_logical, gamma, beta, dx, dgamma, dbeta, mode, G, eps, act, alpha, sa_s, sa_dg, sa_mult, mean=None, var=None,
                    dbias=None):
    """Norm backward whose incoming gradient is the split attention re-weighting's backward mult*s[b][c]*dout + dg[b][c]
    (formed in registers: no usseg_splitattn_apply_bwd_dy pass, no dy tensor)."""
    B, H, W, Cphys, ldx = geom(x)
    d = NormDesc(B * H * W, C_logical, Cphys, ldx, geom(dout)[4], G, mode, eps, act, alpha, geom(dx)[4])
    gamma, beta, mean, var = (_readable(t, Cphys) for t in (gamma, beta, mean, var))
    L.check(L.load().usseg_norm_act_bwd_sa(C.byref(d), x.data_ptr(), dout.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(mean), _ptr(var), B,
                                           sa_s.data_ptr(), sa_dg.data_ptr(), sa_mult, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                           _ptr(dbias), reduce_ws(x.device).data_ptr(), _stream()), "norm_act_bwd_sa")
    return dx


def norm_act_bwd_pair(xa, dya, Ca, gamma_a, beta_a, dxa, dgamma_a, dbeta_a, dbias_a, xb, doutb, Cb, Gb, gamma_b, beta_b, dxb, dgamma_b, dbeta_b,
                      dbias_b, sa_s, sa_dg, sa_mult, eps, alpha) -> bool:
    """A plain LayerNormalization + LeakyReLU backward (A: one group) and one with the split-attention re-weighting folded in (B: ``Gb`` groups, as
    ``norm_act_bwd_sa``) as ONE launch; False - nothing launched - when the pair has no fused instantiation (the caller makes the two calls)."""
    Ba, Ha, Wa, Cpa, ldxa = geom(xa)
    Bb, Hb, Wb, Cpb, ldxb = geom(xb)
    da = NormDesc(Ba * Ha * Wa, Ca, Cpa, ldxa, geom(dya)[4], 1, 0, eps, ACT_LRELU, alpha, geom(dxa)[4])
    db = NormDesc(Bb * Hb * Wb, Cb, Cpb, ldxb, geom(doutb)[4], Gb, 0, eps, ACT_LRELU, alpha, geom(dxb)[4])
    gamma_a, beta_a, gamma_b, beta_b = (_readable(t, n) for t, n in ((gamma_a, Cpa), (beta_a, Cpa), (gamma_b, Cpb), (beta_b, Cpb)))
    rc = L.load().usseg_norm_act_bwd_pair(C.byref(da), xa.data_ptr(), dya.data_ptr(), gamma_a.data_ptr(), beta_a.data_ptr(), dxa.data_ptr(),
                                          dgamma_a.data_ptr(), dbeta_a.data_ptr(), dbias_a.data_ptr(), C.byref(db), xb.data_ptr(), doutb.data_ptr(),
                                          gamma_b.data_ptr(), beta_b.data_ptr(), Bb, sa_s.data_ptr(), sa_dg.data_ptr(), float(sa_mult), dxb.data_ptr(),
                                          dgamma_b.data_ptr(), dbeta_b.data_ptr(), dbias_b.data_ptr(), reduce_ws(xa.device).data_ptr(), _stream())
    if rc == L.ERR_UNSUPPORTED:
        return False
    L.check(rc, "norm_act_bwd_pair")
    return True


def norm_act_bwd(x, dy, C_logical, gamma, beta, dx, dgamma, dbeta, mode, G=1, eps=1e-3, act=ACT_NONE, alpha=0.0, mean=None,
                 var=None, dbias=None, mask=None):
    B, H, W, Cphys, ldx = geom(x)
    lddy = geom(dy)[4]
    d = NormDesc(B * H * W, C_logical, Cphys, ldx, lddy, G, mode, eps, act, alpha, geom(dx)[4])
    gamma, beta, mean, var = (_readable(t, Cphys) for t in (gamma, beta, mean, var))
    ldm = geom(mask)[4] if mask is not None else 0
    L.check(L.load().usseg_norm_act_bwd(C.byref(d), x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(mean),
                                        _ptr(var), _ptr(mask), ldm, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dbias),
                                        reduce_ws(x.device).data_ptr(), _stream()), "norm_act_bwd")
    return dx


def accuracy(probs, y_true, acc):
    """acc[0] = mean over the pixels of argmax(probs) == argmax(y_true) (TBI_ResNest.py:48-51); ``acc``: fp32 [ACC_FLOATS], zeroed once."""
    assert acc.numel() >= ACC_FLOATS and probs.is_contiguous() and y_true.is_contiguous() and probs.dtype == y_true.dtype == torch.float32
    C_ = probs.shape[-1]
    L.check(L.load().usseg_accuracy(probs.data_ptr(), y_true.data_ptr(), probs.numel() // C_, C_, acc.data_ptr(), _stream()), "accuracy")
    return acc[0]


def seg_counts(y_true, probs, counts, round=True, num_classes=3):
    """counts += the metric counters of one batch (usseg_seg_counts: TP / FP / FN, the same over the last image column, the
    confusion matrix, invalid elements; include/usseg.h).  y_true, probs: contiguous fp32 [B,H,W,C] on the device; ``counts``:
    int64 [SEG_COUNTS] on the same device, zeroed by the caller.  One launch, no host synchronisation."""
    assert y_true.shape == probs.shape and y_true.dim() == 4, (tuple(y_true.shape), tuple(probs.shape))
    assert y_true.dtype == probs.dtype == torch.float32 and y_true.is_contiguous() and probs.is_contiguous()
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= L.SEG_COUNTS
    if not (y_true.is_cuda and probs.is_cuda and counts.is_cuda):
        raise RuntimeError("seg_counts: device tensors only (there is no CPU fallback)")
    B, H, W, C_ = y_true.shape
    d = L.SegCountDesc(B, H, W, C_, int(num_classes), int(bool(round)))
    L.check(L.load().usseg_seg_counts(C.byref(d), y_true.data_ptr(), probs.data_ptr(), counts.data_ptr(), _stream()), "seg_counts")
    return counts


# ------------------------------------------------------------------------------------------------ brain-mask cascade (cascade.hip)
def cascade_gate(probs, x, out=None, mask=None):
    """The brain-mask gate (TBIEvaluator.py:221-231): rows of the bf16 input ``x`` [B,H,W,ldx] (``cast_input``'s output) whose mask-model
    probability p0 = ``probs[..., 0]`` rounds to 1 (p0 > 0.5) become zeros in ``out``, the others are copied.  ``out`` defaults to a new
    tensor; ``out is x`` gates in place.  ``mask``: optional uint8 [B,H,W] that receives the gate.  -> ``out``."""
    B, H, W, Cm = probs.shape
    assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.is_cuda
    assert x.dtype == BF16 and x.is_contiguous() and tuple(x.shape[:3]) == (B, H, W), (tuple(x.shape), tuple(probs.shape))
    out = torch.empty_like(x) if out is None else out
    assert out.dtype == BF16 and out.is_contiguous() and out.shape == x.shape
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (B, H, W)
    L.check(L.load().usseg_cascade_gate(probs.data_ptr(), Cm, B * H * W, x.data_ptr(), x.shape[3], out.data_ptr(), _ptr(mask), _stream()),
            "cascade_gate")
    return out


def cascade_maps(probs, prob_map=None, bleed_prob=None):
    """The evaluator's maps of the bleed model's fp32 probabilities [B,H,W,3]: prob_map = ((1 - p0) - 0.5*p1) + p2 (TBIEvaluator.py:249-252)
    and bleed_prob = p2 (:239), each fp32 [B,H,W].  -> (prob_map, bleed_prob)."""
    B, H, W, Cc = probs.shape
    assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.is_cuda
    prob_map = torch.empty((B, H, W), dtype=torch.float32, device=probs.device) if prob_map is None else prob_map
    bleed_prob = torch.empty((B, H, W), dtype=torch.float32, device=probs.device) if bleed_prob is None else bleed_prob
    for t in (prob_map, bleed_prob):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, H, W)
    L.check(L.load().usseg_cascade_maps(probs.data_ptr(), Cc, B * H * W, prob_map.data_ptr(), bleed_prob.data_ptr(), _stream()),
            "cascade_maps")
    return prob_map, bleed_prob


# ------------------------------------------------------------------------------------------------ ensembles and calibration (ensemble.hip)
def _probs4(t, what):
    if not (torch.is_tensor(t) and t.dim() == 4 and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{what}: expected a contiguous fp32 tensor [B,H,W,C], got {getattr(t, 'dtype', type(t).__name__)} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: device tensors only (there is no CPU fallback)")
    return t


def _out_like(t, shape, dtype, ref, what):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=ref.device)
    if not (t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == ref.device):
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor {tuple(shape)} on {ref.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def ensemble_merge(members, flip_w=0, *, variance=True, mean_probs=None, entropy=None, mutual_info=None, variance_out=None):
    """Merge K member probability tensors (fp32 [B,H,W,C], one device, 1 <= K <= 16) in one launch (usseg_ensemble_merge; include/usseg.h):
    the mean, the predictive entropy, the mutual information and - with ``variance`` - the per-class variance.  Bit k of ``flip_w``: member k was
    computed on the left-right mirrored input and is un-mirrored as it is read.  -> (mean_probs, entropy, mutual_info, variance or None)."""
    members = list(members)
    if not 1 <= len(members) <= L.ENSEMBLE_MAX:
        raise ValueError(f"ensemble_merge: 1..{L.ENSEMBLE_MAX} members, got {len(members)}")
    first = _probs4(members[0], "ensemble_merge")
    for m in members[1:]:
        if _probs4(m, "ensemble_merge").shape != first.shape or m.device != first.device:
            raise ValueError(f"ensemble_merge: members differ: {tuple(m.shape)} on {m.device}, {tuple(first.shape)} on {first.device}")
    flip_w = int(flip_w)
    if flip_w < 0 or flip_w >> len(members):
        raise ValueError(f"ensemble_merge: flip_w {flip_w:#x} has bits outside the {len(members)} members")
    B, H, W, C_ = first.shape
    mean_probs = _out_like(mean_probs, first.shape, torch.float32, first, "ensemble_merge mean_probs")
    entropy = _out_like(entropy, (B, H, W), torch.float32, first, "ensemble_merge entropy")
    mutual_info = _out_like(mutual_info, (B, H, W), torch.float32, first, "ensemble_merge mutual_info")
    var = _out_like(variance_out, first.shape, torch.float32, first, "ensemble_merge variance") if variance or variance_out is not None else None
    d = L.EnsembleDesc(B, H, W, C_, len(members))
    ptrs = (C.c_void_p * len(members))(*[m.data_ptr() for m in members])
    L.check(L.load().usseg_ensemble_merge(C.byref(d), ptrs, flip_w, mean_probs.data_ptr(), entropy.data_ptr(), mutual_info.data_ptr(), _ptr(var),
                                          _stream()), "ensemble_merge")
    return mean_probs, entropy, mutual_info, var


def ensemble_image_scores(mean_probs, entropy, mutual_info, scores=None, counts=None):
    """Per image: the mean entropy, the mean and the maximum mutual information, and the mean entropy over the pixels predicted as the last
    class (usseg_ensemble_image_scores).  -> (scores fp32 [B,4], counts int32 [B]: those pixels).  One launch, bitwise reproducible."""
    _probs4(mean_probs, "ensemble_image_scores")
    B, H, W, C_ = mean_probs.shape
    for t, n in ((entropy, "entropy"), (mutual_info, "mutual_info")):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, H, W) and t.device == mean_probs.device):
            raise ValueError(f"ensemble_image_scores: {n} must be a contiguous fp32 [B,H,W] tensor beside mean_probs {tuple(mean_probs.shape)}")
    scores = _out_like(scores, (B, 4), torch.float32, mean_probs, "ensemble_image_scores scores")
    counts = _out_like(counts, (B,), torch.int32, mean_probs, "ensemble_image_scores counts")
    d = L.EnsembleDesc(B, H, W, C_, 1)
    L.check(L.load().usseg_ensemble_image_scores(C.byref(d), mean_probs.data_ptr(), entropy.data_ptr(), mutual_info.data_ptr(), scores.data_ptr(),
                                                 counts.data_ptr(), _stream()), "ensemble_image_scores")
    return scores, counts


def calibration_bins(probs, y_true, counts, bins=15, cls=-1):
    """counts += the reliability counters of one batch (usseg_calibration_bins): per confidence bin the pixels, the hits and the sum of
    rint(conf * 2^24), then the Brier sum in the same units and the invalid pixels.  probs, y_true: contiguous fp32 [B,H,W,C] on the device;
    ``counts``: int64 [bins*3 + 2] there, zeroed by the caller.  ``cls`` -1: top-label calibration, k: class k.  One launch, no host sync."""
    _probs4(probs, "calibration_bins")
    if _probs4(y_true, "calibration_bins").shape != probs.shape or y_true.device != probs.device:
        raise ValueError(f"calibration_bins: probs {tuple(probs.shape)} and y_true {tuple(y_true.shape)} differ")
    bins, cls = int(bins), int(cls)
    if not 1 <= bins <= L.CALIB_MAX_BINS:
        raise ValueError(f"calibration_bins: 1..{L.CALIB_MAX_BINS} bins, got {bins}")
    B, H, W, C_ = probs.shape
    if not -1 <= cls < C_:
        raise ValueError(f"calibration_bins: cls must be -1 or a class below {C_}, got {cls}")
    if not (torch.is_tensor(counts) and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == bins * 3 + 2
            and counts.device == probs.device):
        raise ValueError(f"calibration_bins: counts must be a contiguous int64 tensor of {bins * 3 + 2} elements on {probs.device}")
    d = L.CalibDesc(B, H, W, C_, bins, cls)
    L.check(L.load().usseg_calibration_bins(C.byref(d), probs.data_ptr(), y_true.data_ptr(), counts.data_ptr(), _stream()), "calibration_bins")
    return counts


# ------------------------------------------------------------------------------------------------ operating points (operating_point.hip)
def _counts_i64(counts, n, ref, what):
    if not (torch.is_tensor(counts) and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == n and counts.device == ref.device):
        raise ValueError(f"{what}: counts must be a contiguous int64 tensor of {n} elements on {ref.device}")


def score_sweep(probs, y_true, counts, bins=1024, cls=-1):
    """counts += the sweep counters of one batch (usseg_score_sweep): per score bin of class ``cls`` the negatives and the positives, then the
    invalid pixels.  probs, y_true: contiguous fp32 [B,H,W,C] on the device; ``counts``: int64 [2*bins + 1] there, zeroed by the caller.
    ``bins``: a power of two in 2..4096; a negative ``cls`` counts from the last class.  One launch, no host sync."""
    bins, cls = int(bins), int(cls)
    if not 2 <= bins <= L.SWEEP_MAX_BINS or bins & (bins - 1):
        raise ValueError(f"score_sweep: bins must be a power of two in 2..{L.SWEEP_MAX_BINS}, got {bins}")
    _probs4(probs, "score_sweep")
    if _probs4(y_true, "score_sweep").shape != probs.shape or y_true.device != probs.device:
        raise ValueError(f"score_sweep: probs {tuple(probs.shape)} and y_true {tuple(y_true.shape)} differ")
    B, H, W, C_ = probs.shape
    if not -C_ <= cls < C_:
        raise ValueError(f"score_sweep: cls must be a class below {C_} (or negative, from the last), got {cls}")
    _counts_i64(counts, 2 * bins + 1, probs, "score_sweep")
    if probs.numel() == 0:                        # an empty batch has no storage to point at: nothing to count, nothing launched
        return counts
    d = L.SweepDesc(B, H, W, C_, bins, cls % C_)
    L.check(L.load().usseg_score_sweep(C.byref(d), probs.data_ptr(), y_true.data_ptr(), counts.data_ptr(), _stream()), "score_sweep")
    return counts


def _beta_list(betas, what):
    betas = [float(b) for b in (betas.tolist() if hasattr(betas, "tolist") else betas)]
    if not 1 <= len(betas) <= L.TEMP_MAX_BETAS:
        raise ValueError(f"{what}: 1..{L.TEMP_MAX_BETAS} betas, got {len(betas)}")
    for b in betas:
        if not 0.0 < b <= 16.0:                   # (a NaN compares false)
            raise ValueError(f"{what}: every beta must be finite with 0 < beta <= 16, got {b!r}")
    return betas


def temperature_nll(probs, y_true, betas, counts):
    """counts[j] += sum over the valid pixels of rint(nll_j * 2^20), nll_j the negative log-likelihood of the label under
    softmax(betas[j] * log(probs + 1e-7)); counts[n] += the valid, counts[n+1] += the invalid pixels (usseg_temperature_nll).  ``betas``: 1..16
    host floats in (0, 16], rounded to fp32; ``counts``: int64 [len(betas) + 2] on the device.  One launch for every candidate, no host sync."""
    betas = _beta_list(betas, "temperature_nll")
    _probs4(probs, "temperature_nll")
    if _probs4(y_true, "temperature_nll").shape != probs.shape or y_true.device != probs.device:
        raise ValueError(f"temperature_nll: probs {tuple(probs.shape)} and y_true {tuple(y_true.shape)} differ")
    _counts_i64(counts, len(betas) + 2, probs, "temperature_nll")
    B, H, W, C_ = probs.shape
    if probs.numel() == 0:
        return counts
    d = L.TempDesc(B, H, W, C_, len(betas))
    arr = (C.c_float * len(betas))(*betas)
    L.check(L.load().usseg_temperature_nll(C.byref(d), probs.data_ptr(), y_true.data_ptr(), arr, counts.data_ptr(), _stream()), "temperature_nll")
    return counts


def apply_temperature(probs, beta, out=None):
    """softmax(beta * log(probs + 1e-7)) per pixel (usseg_apply_temperature).  ``beta``: a one-element fp32 DEVICE tensor (1 / temperature) the
    kernel reads when it runs, so a captured graph follows it.  ``out`` may be ``probs``.  One launch, no host sync."""
    _probs4(probs, "apply_temperature")
    if not (torch.is_tensor(beta) and beta.dtype == torch.float32 and beta.numel() == 1 and beta.device == probs.device):
        raise ValueError(f"apply_temperature: beta must be a one-element fp32 tensor on {probs.device}")
    out = _out_like(out, probs.shape, torch.float32, probs, "apply_temperature out")
    B, H, W, C_ = probs.shape
    if probs.numel() == 0:
        return out
    d = L.TempDesc(B, H, W, C_, 1)
    L.check(L.load().usseg_apply_temperature(C.byref(d), probs.data_ptr(), beta.data_ptr(), out.data_ptr(), _stream()), "apply_temperature")
    return out


def norm_act_bwd_res(x, dy, C_logical, gamma, beta, dres, dx, dgamma, dbeta, eps, dbias=None):
    """Plain LayerNormalization backward + the residual branch of a pre-norm block: dx = bf16(bf16(LN'(dy)) + dres) in one pass;
    ``dbias`` += the column sums of the stored dx."""
    B, H, W, Cphys, ldx = geom(x)
    d = NormDesc(B * H * W, C_logical, Cphys, ldx, geom(dy)[4], 1, 0, eps, ACT_NONE, 0.0, geom(dx)[4])
    L.check(L.load().usseg_norm_act_bwd_res(C.byref(d), x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dres.data_ptr(),
                                            geom(dres)[4], dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dbias),
                                            reduce_ws(x.device).data_ptr(), _stream()), "norm_act_bwd_res")
    return dx


def bn_act_pool_fwd(x, C_logical, gamma, beta, mean, var, eps, act, alpha, out=None):
    """inference BatchNorm + activation + AveragePooling2D(2,2) in one pass: x [B,H,W,Cp] -> [B,H/2,W/2,Cp]."""
    B, H, W, Cp, ldx = geom(x)
    out = out if out is not None else new_act(B, H // 2, W // 2, Cp, x.device)
    L.check(L.load().usseg_bn_act_pool_fwd(x.data_ptr(), B, H, W, C_logical, Cp, ldx, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                           eps, act, alpha, out.data_ptr(), geom(out)[4], _stream()), "bn_act_pool_fwd")
    return out


def bn_act_pool_bwd(x, dy, C_logical, gamma, beta, mean, var, eps, act, alpha, dx, dgamma, dbeta, dbias=None):
    B, H, W, Cp, ldx = geom(x)
    L.check(L.load().usseg_bn_act_pool_bwd(x.data_ptr(), dy.data_ptr(), B, H, W, C_logical, Cp, ldx, geom(dy)[4], gamma.data_ptr(), beta.data_ptr(),
                                           mean.data_ptr(), var.data_ptr(), eps, act, alpha, dx.data_ptr(), geom(dx)[4], dgamma.data_ptr(),
                                           dbeta.data_ptr(), _ptr(dbias), reduce_ws(x.device).data_ptr(), _stream()), "bn_act_pool_bwd")
    return dx


def dropout_mask(mask, seed: int, rate: float, step_dev=None):
    """``step_dev``: int32 device counter mixed into the seed (fresh masks when the launch is replayed from a HIP graph)."""
    B, H, W, Cc, ld = geom(mask)
    if step_dev is not None:
        L.check(L.load().usseg_dropout_mask_step(mask.data_ptr(), B * H * W, Cc, ld, seed, step_dev.data_ptr(), rate, _stream()), "dropout_mask_step")
        return mask
    L.check(L.load().usseg_dropout_mask(mask.data_ptr(), B * H * W, Cc, ld, seed, rate, _stream()), "dropout_mask")
    return mask


def counter_add(counter, inc: int = 1):
    """counter (int32 device tensor) += inc, one launch (capturable)."""
    assert counter.dtype == torch.int32
    L.check(L.load().usseg_counter_add(counter.data_ptr(), inc, _stream()), "counter_add")


def channel_stats(x, C_logical, s, s2):
    B, H, W, _, ldx = geom(x)
    L.check(L.load().usseg_channel_stats(x.data_ptr(), B * H * W, C_logical, ldx, s.data_ptr(), s2.data_ptr(),
                                         reduce_ws(x.device).data_ptr(), _stream()), "channel_stats")


def bn_finalize_stats(s, s2, M, C_logical, momentum, mean, var, moving_mean=None, moving_var=None):
    L.check(L.load().usseg_bn_finalize_stats(s.data_ptr(), s2.data_ptr(), M, C_logical, momentum, mean.data_ptr(), var.data_ptr(),
                                             _ptr(moving_mean), _ptr(moving_var), _stream()), "bn_finalize_stats")


def bn_batch_stats(x, C_logical, momentum, mean, var, moving_mean=None, moving_var=None):
    """mean / var (overwritten) = the batch mean and biased variance of x's channels; the moving statistics move with momentum."""
    B, H, W, _, ldx = geom(x)
    L.check(L.load().usseg_bn_batch_stats(x.data_ptr(), B * H * W, C_logical, ldx, momentum, mean.data_ptr(), var.data_ptr(), _ptr(moving_mean),
                                          _ptr(moving_var), reduce_ws(x.device).data_ptr(), _stream()), "bn_batch_stats")


def bn_train_bwd_fix(x, dx, C_logical, gamma, mean, var, eps, tg, tb):
    B, H, W, Cphys, ldx = geom(x)
    L.check(L.load().usseg_bn_train_bwd_fix(x.data_ptr(), dx.data_ptr(), B * H * W, C_logical, Cphys, ldx, geom(dx)[4], gamma.data_ptr(),
                                            mean.data_ptr(), var.data_ptr(), eps, tg.data_ptr(), tb.data_ptr(), _stream()), "bn_train_bwd_fix")


def act_fwd(x, out, act, alpha):
    B, H, W, Cc, ldx = geom(x)
    L.check(L.load().usseg_act_fwd(x.data_ptr(), B * H * W, Cc, ldx, geom(out)[4], act, alpha, out.data_ptr(), _stream()), "act_fwd")
    return out


def act_bwd(x, dy, dx, act, alpha):
    B, H, W, Cc, ldx = geom(x)
    L.check(L.load().usseg_act_bwd(x.data_ptr(), dy.data_ptr(), B * H * W, Cc, ldx, geom(dy)[4], geom(dx)[4], act, alpha,
                                   dx.data_ptr(), _stream()), "act_bwd")
    return dx


def act_bwd_colsum(x, dy, dx, act, alpha, db, C_logical):
    """act_bwd + the column sums of its output into ``db`` (the producing conv's bias gradient) in one pass."""
    B, H, W, Cc, ldx = geom(x)
    L.check(L.load().usseg_act_bwd_colsum(x.data_ptr(), dy.data_ptr(), B * H * W, C_logical, ldx, geom(dy)[4], geom(dx)[4], act, alpha, dx.data_ptr(),
                                          db.data_ptr(), reduce_ws(x.device).data_ptr(), _stream()), "act_bwd_colsum")
    return dx


def avgpool2_fwd(x, out):
    B, H, W, Cc, ldx = geom(x)
    L.check(L.load().usseg_avgpool2_fwd(x.data_ptr(), B, H, W, Cc, ldx, geom(out)[4], out.data_ptr(), _stream()), "avgpool2_fwd")
    return out


def avgpool2_bwd(dy, dx, add=None, db=None):
    """``db``: optional fp32 vector to which the column sums of the stored dx are ADDED (the bias gradient of the conv in front of the pool).
    Up to 512 channels one fused kernel writes dx and the sums; wider rows (up to colsum's 16384 channels) take the plain backward followed by a
    ``colsum`` launch over dx - the same sums, added to ``db`` in the same way."""
    B, H, W, Cc, lddx = geom(dx)
    ldadd = geom(add)[4] if add is not None else 0
    if db is not None and Cc <= 512:
        L.check(L.load().usseg_avgpool2_bwd_colsum(dy.data_ptr(), B, H, W, Cc, geom(dy)[4], lddx, _ptr(add), ldadd, dx.data_ptr(), db.data_ptr(),
                                                   reduce_ws(dx.device).data_ptr(), _stream()), "avgpool2_bwd_colsum")
        return dx
    L.check(L.load().usseg_avgpool2_bwd(dy.data_ptr(), B, H, W, Cc, geom(dy)[4], lddx, _ptr(add), ldadd, dx.data_ptr(),
                                        _stream()), "avgpool2_bwd")
    if db is not None:      # rows wider than the fused kernel's 512 channels: the column sums of the stored dx in a launch of their own
        colsum(dx, db)
    return dx


def copy_channels(src, dst, accumulate=False):
    B, H, W, Cc, lds = geom(src)
    Bd, Hd, Wd, Cd, ldd = geom(dst)
    assert B * H * W == Bd * Hd * Wd and Cc == Cd
    L.check(L.load().usseg_copy_channels(src.data_ptr(), B * H * W, Cc, lds, dst.data_ptr(), ldd, 1 if accumulate else 0,
                                         _stream()), "copy_channels")
    return dst


def cast_input(x: torch.Tensor, Cphys: int) -> torch.Tensor:
    """fp32/fp64 NHWC device tensor -> bf16 [B,H,W,Cphys] (zero pad channels)."""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.float64)
    B, H, W, Cc = x.shape
    out = new_act(B, H, W, Cphys, x.device)
    L.check(L.load().usseg_cast_input(x.data_ptr(), 1 if x.dtype == torch.float64 else 0, B * H * W, Cc, out.data_ptr(), Cphys,
                                      _stream()), "cast_input")
    return out


def to_f32(x: torch.Tensor, C_logical: Optional[int] = None) -> torch.Tensor:
    B, H, W, Cc, ld = geom(x)
    Cl = C_logical or Cc
    out = torch.empty((B, H, W, Cl), dtype=torch.float32, device=x.device)
    L.check(L.load().usseg_cast_bf16_to_f32(x.data_ptr(), B * H * W, Cl, ld, out.data_ptr(), _stream()), "cast_bf16_to_f32")
    return out


def colsum(dy, db: torch.Tensor, C_logical: Optional[int] = None):
    B, H, W, Cc, ld = geom(dy)
    L.check(L.load().usseg_colsum(dy.data_ptr(), B * H * W, C_logical or Cc, ld, db.data_ptr(), reduce_ws(dy.device).data_ptr(),
                                  _stream()), "colsum")


# ------------------------------------------------------------------------------------------------ optimiser helpers
def fill_f32(t: torch.Tensor, value: float = 0.0):
    assert t.dtype == torch.float32 and t.is_contiguous()
    L.check(L.load().usseg_fill_f32(t.data_ptr(), t.numel(), value, _stream()), "fill_f32")


def sumsq(g: torch.Tensor, out: torch.Tensor):
    assert out.numel() >= ACC_FLOATS, "sumsq accumulates through a USSEG_ACC_FLOATS buffer"
    L.check(L.load().usseg_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), _stream()), "sumsq")


def sum_f32(x: torch.Tensor, out: torch.Tensor):
    """out[0] = sum(x) (fp32, contiguous) through an ACC_FLOATS accumulator (zeroed once): fixed-order, no framework reduction."""
    assert out.numel() >= ACC_FLOATS and x.dtype == torch.float32 and x.is_contiguous()
    L.check(L.load().usseg_sum_f32(x.data_ptr(), x.numel(), out.data_ptr(), _stream()), "sum_f32")
    return out[0]


def sumsq_advance(g: torch.Tensor, out: torch.Tensor, step_dev, lr_t_dev, lr, b1, b2):
    """sumsq + adam_advance in ONE launch (the last workgroup of the ordered sum moves the step counter on)."""
    assert out.numel() >= ACC_FLOATS
    L.check(L.load().usseg_sumsq_advance(g.data_ptr(), g.numel(), out.data_ptr(), step_dev.data_ptr(), lr_t_dev.data_ptr(), lr, b1, b2, _stream()),
            "sumsq_advance")


def reinject_hidden(hidden: torch.Tensor, views, backward: bool):
    """Decoder.py:140-141 for all scales at once.  ``hidden``: contiguous bf16 tensor; ``views``: channel-slice views
    [B,h_i,w_i,c0_i] of the concat buffers (forward: written; backward: their gradients, summed into ``hidden``)."""
    assert hidden.is_contiguous() and hidden.dtype == BF16 and 1 <= len(views) <= 4
    n = len(views)
    bufs = (C.c_void_p * n)(*[v.data_ptr() for v in views])
    c0 = (C.c_int32 * n)(*[v.shape[3] for v in views])
    ld = (C.c_int32 * n)(*[geom(v)[4] for v in views])
    for v in views:
        assert v.numel() == hidden.numel()
    L.check(L.load().usseg_reinject_hidden(hidden.data_ptr(), hidden.numel(), n, bufs, c0, ld, 1 if backward else 0, _stream()), "reinject_hidden")


def scale_by_clip(g: torch.Tensor, sumsq_t: torch.Tensor, clip_norm: float):
    L.check(L.load().usseg_scale_f32(g.data_ptr(), g.numel(), sumsq_t.data_ptr(), clip_norm, _stream()), "scale_f32")


def adam_clip_step(p, g, m, v, sumsq_t, clip_norm, lr_t_dev, b1, b2, eps):
    L.check(L.load().usseg_adam_clip_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), _ptr(sumsq_t),
                                          clip_norm, lr_t_dev.data_ptr(), b1, b2, eps, _stream()), "adam_clip_step")


def adam_advance(step_dev, lr_t_dev, lr, b1, b2):
    L.check(L.load().usseg_adam_advance(step_dev.data_ptr(), lr_t_dev.data_ptr(), lr, b1, b2, _stream()), "adam_advance")


def sched_advance(step_dev, sched_dev, lr_t_dev, wd_t_dev, b1, b2):
    """step += 1 with lr_t / wd_t of the schedule piece of the step BEFORE the increment, read from the device table ``sched_dev``."""
    L.check(L.load().usseg_sched_advance(step_dev.data_ptr(), sched_dev.data_ptr(), lr_t_dev.data_ptr(), wd_t_dev.data_ptr(), b1, b2, _stream()),
            "sched_advance")


def sumsq_sched_advance(g: torch.Tensor, out: torch.Tensor, step_dev, sched_dev, lr_t_dev, wd_t_dev, b1, b2):
    """sumsq + sched_advance in ONE launch (the last workgroup of the ordered sum reads the table)."""
    assert out.numel() >= ACC_FLOATS
    L.check(L.load().usseg_sumsq_sched_advance(g.data_ptr(), g.numel(), out.data_ptr(), step_dev.data_ptr(), sched_dev.data_ptr(), lr_t_dev.data_ptr(),
                                               wd_t_dev.data_ptr(), b1, b2, _stream()), "sumsq_sched_advance")


def adamw_step(p, g, m, v, sumsq_t, clip_norm, lr_t_dev, wd_t_dev, decay_mask, b1, b2, eps):
    """Decoupled weight decay (p -= wd_t*p where ``decay_mask`` is nonzero, or everywhere if it is None) then the Adam update."""
    L.check(L.load().usseg_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), _ptr(sumsq_t), clip_norm,
                                      lr_t_dev.data_ptr(), wd_t_dev.data_ptr(), _ptr(decay_mask), b1, b2, eps, _stream()), "adamw_step")


# UssegAverage as int32 words: mode, decay bits, dynamic_decay, start, period (usseg.h; flat.AdamClip keeps it on the device)
AVERAGE_MODES = {"ema": L.AVERAGE_EMA, "swa": L.AVERAGE_SWA}
AVERAGE_WORDS = C.sizeof(L.Average) // 4


def adamw_avg_step(p, g, m, v, avg, sumsq_t, clip_norm, lr_t_dev, wd_t_dev, decay_mask, b1, b2, eps, step_dev, avg_desc):
    """``adamw_step`` (``wd_t_dev`` None: no decay, the fixed-rate arithmetic) and the EMA / SWA average of the updated ``p`` in one launch;
    the blend coefficient comes from the device descriptor ``avg_desc`` at the device step counter."""
    assert avg.dtype == torch.float32 and avg.numel() == p.numel() and avg_desc.numel() >= AVERAGE_WORDS
    L.check(L.load().usseg_adamw_avg_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), avg.data_ptr(), p.numel(), _ptr(sumsq_t),
                                          clip_norm, lr_t_dev.data_ptr(), _ptr(wd_t_dev), _ptr(decay_mask), b1, b2, eps, step_dev.data_ptr(),
                                          avg_desc.data_ptr(), _stream()), "adamw_avg_step")


def average_update(avg, p, step_dev, avg_desc):
    """The average alone (``p`` updated elsewhere): the same bits of ``avg`` as ``adamw_avg_step``."""
    assert avg.dtype == torch.float32 and p.dtype == torch.float32 and avg.numel() == p.numel() and avg_desc.numel() >= AVERAGE_WORDS
    L.check(L.load().usseg_average_update(avg.data_ptr(), p.data_ptr(), p.numel(), step_dev.data_ptr(), avg_desc.data_ptr(), _stream()),
            "average_update")


def swap_f32(a: torch.Tensor, b: torch.Tensor):
    """Exchanges two disjoint contiguous fp32 buffers in place."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    L.check(L.load().usseg_swap_f32(a.data_ptr(), b.data_ptr(), a.numel(), _stream()), "swap_f32")


def grad_accumulate(acc: torch.Tensor, grad: torch.Tensor, finish: bool, divisor: float):
    """One micro-batch gradient into the accumulator.  ``finish`` False: ``acc += grad``.  True: ``grad = (acc + grad) / divisor`` and
    ``acc = 0`` - every operation one rounded fp32 operation (usseg_accumulate.h), ``divisor`` the number of micro-steps of a group."""
    assert acc.dtype == torch.float32 and grad.dtype == torch.float32 and acc.is_contiguous() and grad.is_contiguous()
    assert acc.numel() == grad.numel()
    L.check(L.load().usseg_grad_accumulate(acc.data_ptr(), grad.data_ptr(), acc.numel(), 1 if finish else 0, float(divisor), _stream()),
            "grad_accumulate")


# ------------------------------------------------------------------------------------------------ fused stem
def stem_fwd(x, w1, b1, w2, b2, w3, b3, gamma, beta, mean, var, eps, alpha):
    """ResNest.py:39-47 in one launch -> (y1 [B,H,W,16], t1 [B,H,W,32], c2 [B,H,W,32] pre-norm, pooled [B,H/2,W/2,32])."""
    B, H, W, Cin, ldx = geom(x)
    assert Cin == 8 and x.dtype == BF16
    dev = x.device
    y1, t1, c2 = new_act(B, H, W, 16, dev), new_act(B, H, W, 32, dev), new_act(B, H, W, 32, dev)
    pooled = new_act(B, H // 2, W // 2, 32, dev)
    L.check(L.load().usseg_stem_fwd(B, H, W, x.data_ptr(), ldx, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                                    b3.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), eps, alpha,
                                    y1.data_ptr(), t1.data_ptr(), c2.data_ptr(), pooled.data_ptr(), _stream()), "stem_fwd")
    return y1, t1, c2, pooled


def stem_fwd_infer(x, w1, b1, w2, b2, w3, b3, gamma, beta, mean, var, eps, alpha):
    """``stem_fwd`` without the tensors of the backward pass -> pooled [B,H/2,W/2,32], bit-identical to ``stem_fwd``'s."""
    B, H, W, Cin, ldx = geom(x)
    assert Cin == 8 and x.dtype == BF16
    pooled = new_act(B, H // 2, W // 2, 32, x.device)
    L.check(L.load().usseg_stem_fwd_infer(B, H, W, x.data_ptr(), ldx, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                                          b3.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), eps, alpha,
                                          pooled.data_ptr(), _stream()), "stem_fwd_infer")
    return pooled


def conv3_dgrad_actbwd(dy, wd, yact, dx, mode, alpha, dbias, gamma=None, beta=None, var=None, eps=1e-3, dgamma=None, dbeta=None) -> bool:
    """3x3 backward-data of a 32-output-channel stem conv + the backward of the layer in front of it in one launch: mode 2 = folded inference
    BatchNorm + LeakyReLU from the activated tensor ``yact`` (32 channels), mode 0 = LeakyReLU + column sums (16 channels).  False - nothing
    launched - when there is no fused kernel for the shape."""
    B, H, W, Cdy, lddy = geom(dy)
    Co = yact.shape[-1]
    if Cdy != 32 or tuple(wd.shape) != (roundup(Co, 16), 9 * 32):
        return False
    rc = L.load().usseg_conv3_dgrad_actbwd(B, H, W, dy.data_ptr(), lddy, wd.data_ptr(), Co, yact.data_ptr(), geom(yact)[4], mode, _ptr(gamma), _ptr(beta),
                                           _ptr(var), eps, alpha, dx.data_ptr(), geom(dx)[4], _ptr(dgamma), _ptr(dbeta), dbias.data_ptr(),
                                           reduce_ws(dy.device).data_ptr(), _stream())
    if rc == -2:
        return False
    L.check(rc, "conv3_dgrad_actbwd")
    return True


# ------------------------------------------------------------------------------------------------ fused cardinal group (K3)
def cardinal_desc(B, H, W, Cin, P, cv11, cvkk, Up, Vp, Oc, ldx, ldu, ldv, ldsc, eps, alpha) -> CardinalDesc:
    return CardinalDesc(B, H, W, Cin, P, cv11, cvkk, Up, Vp, Oc, ldx, ldu, ldv, ldsc, eps, alpha)


def cardinal_supported(Cin, P, cv11, cvkk, Up, Vp, Oc) -> bool:
    d = cardinal_desc(1, 8, 8, Cin, P, cv11, cvkk, Up, Vp, Oc, Cin, Up, Vp, Oc, 1e-3, 0.3)
    return bool(L.load().usseg_cardinal_supported(C.byref(d)))


def cardinal_fwd(x, w1, b1, g1, be1, w2, b2, g2, be2, wsc, bsc, gsc, besc, P, cv11, cvkk, Up, Vp, Oc, eps, alpha):
    """One launch for a residual_S stage's first half (ResNest.py:136-147 for all paths, :99-101): grouped 1x1 -> LN -> LeakyReLU ->
    grouped 3x3 -> LN -> LeakyReLU (+ pooled partial rows) and the shortcut 1x1 -> LN -> LeakyReLU.
    -> (u_raw, u, v_raw, y, gap, sc_raw, sc); gap = (rows [B,tiles,Vp], tiles, Vp) for ``splitattn_fwd(..., gap=gap)``."""
    B, H, W, Cin, ldx = geom(x)
    dev = x.device
    u_raw, u = new_act(B, H, W, Up, dev), new_act(B, H, W, Up, dev)
    v_raw, y = new_act(B, H, W, Vp, dev), new_act(B, H, W, Vp, dev)
    sc_raw, sc = new_act(B, H, W, Oc, dev), new_act(B, H, W, Oc, dev)
    tiles = ((H + 7) // 8) * ((W + 7) // 8)
    rows = torch.empty((B, tiles, Vp), dtype=torch.float32, device=dev)
    d = cardinal_desc(B, H, W, Cin, P, cv11, cvkk, Up, Vp, Oc, ldx, Up, Vp, Oc, eps, alpha)
    g1, be1, g2, be2, gsc, besc = (_readable(t, n) for t, n in ((g1, P * cv11), (be1, P * cv11), (g2, P * cvkk), (be2, P * cvkk), (gsc, Oc), (besc, Oc)))
    L.check(L.load().usseg_cardinal_fwd(C.byref(d), x.data_ptr(), w1.data_ptr(), b1.data_ptr(), g1.data_ptr(), be1.data_ptr(), w2.data_ptr(),
                                        b2.data_ptr(), g2.data_ptr(), be2.data_ptr(), wsc.data_ptr(), bsc.data_ptr(), gsc.data_ptr(), besc.data_ptr(),
                                        u_raw.data_ptr(), u.data_ptr(), v_raw.data_ptr(), y.data_ptr(), rows.data_ptr(), sc_raw.data_ptr(),
                                        sc.data_ptr(), _stream()), "cardinal_fwd")
    return u_raw, u, v_raw, y, (rows, tiles, Vp), sc_raw, sc


def cardinal_fwd_infer(x, w1, b1, g1, be1, w2, b2, g2, be2, wsc, bsc, gsc, besc, P, cv11, cvkk, Up, Vp, Oc, eps, alpha):
    """``cardinal_fwd`` without the tensors of the backward pass -> (y, gap, sc), bit-identical to ``cardinal_fwd``'s."""
    B, H, W, Cin, ldx = geom(x)
    dev = x.device
    y, sc = new_act(B, H, W, Vp, dev), new_act(B, H, W, Oc, dev)
    tiles = ((H + 7) // 8) * ((W + 7) // 8)
    rows = torch.empty((B, tiles, Vp), dtype=torch.float32, device=dev)
    d = cardinal_desc(B, H, W, Cin, P, cv11, cvkk, Up, Vp, Oc, ldx, Up, Vp, Oc, eps, alpha)
    g1, be1, g2, be2, gsc, besc = (_readable(t, n) for t, n in ((g1, P * cv11), (be1, P * cv11), (g2, P * cvkk), (be2, P * cvkk), (gsc, Oc), (besc, Oc)))
    L.check(L.load().usseg_cardinal_fwd_infer(C.byref(d), x.data_ptr(), w1.data_ptr(), b1.data_ptr(), g1.data_ptr(), be1.data_ptr(), w2.data_ptr(),
                                              b2.data_ptr(), g2.data_ptr(), be2.data_ptr(), wsc.data_ptr(), bsc.data_ptr(), gsc.data_ptr(),
                                              besc.data_ptr(), y.data_ptr(), rows.data_ptr(), sc.data_ptr(), _stream()), "cardinal_fwd_infer")
    return y, (rows, tiles, Vp), sc


def cardinal_bwd(dout, dsc, v_raw, u_raw, sc_raw, w2d, g2, be2, g1, be1, gsc, besc, sa_s, sa_dg, sa_mult, dv, dcat, grads, Cin, P, cv11, cvkk, Up,
                 Vp, Oc, eps, alpha):
    """One launch for the backward pass of ``cardinal_fwd``'s chain (GradientTape through ResNest.py:136-147 and :100-101): the split-attention
    re-weighting's backward (``sa_mult*sa_s*dout + sa_dg``) + conv2_bn backward -> ``dv``; grouped 3x3 backward-data; conv1_bn backward ->
    ``dcat[..., :Up]``; shortcut norm backward of ``dsc`` -> ``dcat[..., Up:]``.  ``grads`` = (dg2, dbe2, db2, dg1, dbe1, db1, dgsc, dbesc,
    dbsc) accumulate.  -> (dv, dcat)"""
    B, H, W, _, ldo = geom(dout)
    d = cardinal_desc(B, H, W, Cin, P, cv11, cvkk, Up, Vp, Oc, Cin, geom(u_raw)[4], geom(v_raw)[4], geom(sc_raw)[4], eps, alpha)
    assert geom(dv)[4] == d.ldv and dcat.shape[-1] >= Up + Oc
    g2, be2, g1, be1, gsc, besc = (_readable(t, n) for t, n in ((g2, P * cvkk), (be2, P * cvkk), (g1, P * cv11), (be1, P * cv11), (gsc, Oc), (besc, Oc)))
    L.check(L.load().usseg_cardinal_bwd(C.byref(d), dout.data_ptr(), ldo, dsc.data_ptr(), geom(dsc)[4], v_raw.data_ptr(), u_raw.data_ptr(),
                                        sc_raw.data_ptr(), w2d.data_ptr(), g2.data_ptr(), be2.data_ptr(), g1.data_ptr(), be1.data_ptr(),
                                        gsc.data_ptr(), besc.data_ptr(), sa_s.data_ptr(), sa_dg.data_ptr(), float(sa_mult), dv.data_ptr(),
                                        dcat.data_ptr(), geom(dcat)[4], *[t.data_ptr() for t in grads], reduce_ws(dout.device).data_ptr(),
                                        _stream()), "cardinal_bwd")
    return dv, dcat


# ------------------------------------------------------------------------------------------------ split attention
def splitattn_desc(B, HW, P, R, Cg, Hd, ldy, ldo, Cy_phys, Co_phys, mult, norm_mode, eps, act, alpha, use_sigmoid) -> SplitAttnDesc:
    return SplitAttnDesc(B, HW, P, R, Cg, Hd, ldy, ldo, Cy_phys, Co_phys, mult, norm_mode, eps, act, alpha, 1 if use_sigmoid else 0)


def _sa_params(w1, b1, gamma, beta, mean, var, w2, b2) -> SplitAttnParams:
    return SplitAttnParams(_ptr(w1), _ptr(b1), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), _ptr(w2), _ptr(b2))


def splitattn_fwd(d: SplitAttnDesc, y, params, out, gap=None):
    """params = (w1,b1,gamma,beta,mean,var,w2,b2) fp32 tensors laid out per path.  ``gap``: the pooled partial rows
    (tensor [B,nb,Cphys], nb, Cphys) that ``norm_act_fwd_gap`` produced together with y - without it the pooling pass over y
    runs here.  Returns (out, g, s, ws); g = (tensor, rows, stride) is what ``splitattn_bwd`` takes back."""
    dev = y.device
    Cy = d.P * d.R * d.Cg
    s = torch.empty((d.B, Cy), dtype=torch.float32, device=dev)
    ws = torch.empty(d.B * d.P * (d.Cg + 2 * d.Hd), dtype=torch.float32, device=dev)
    lib = L.load()
    if gap is None:
        g = torch.empty((d.B, Cy), dtype=torch.float32, device=dev)      # overwritten by usseg_splitattn_gap
        L.check(lib.usseg_splitattn_gap(C.byref(d), y.data_ptr(), g.data_ptr(), reduce_ws(dev).data_ptr(), _stream()), "splitattn_gap")
        gap = (g, 1, Cy)
    sp = _sa_params(*params)
    L.check(lib.usseg_splitattn_mlp_fwd(C.byref(d), gap[0].data_ptr(), gap[1], gap[2], C.byref(sp), s.data_ptr(), ws.data_ptr(), _stream()),
            "splitattn_mlp_fwd")
    L.check(lib.usseg_splitattn_apply_fwd(C.byref(d), y.data_ptr(), s.data_ptr(), out.data_ptr(), _stream()), "splitattn_apply_fwd")
    return out, gap, s, ws


def splitattn_bwd(d: SplitAttnDesc, y, dout, params, grads, g, s, ws, dy):
    """grads = (dw1,db1,dgamma,dbeta,dw2,db2) accumulate (per-image partial rows + an ordered finishing reduction).
    ``dy`` tensor: written (dy = mult*s*dout + dg).  ``dy=None``: the re-weighting's backward is left to the caller's
    ``norm_act_bwd_sa`` (R == 1 only) and (s, dg) are returned for it."""
    dev = y.device
    Cy = d.P * d.R * d.Cg
    dg = torch.empty((d.B, Cy), dtype=torch.float32, device=dev)
    lib = L.load()
    lddo = geom(dout)[4]
    if not isinstance(g, tuple):
        g = (g, 1, Cy)
    sp = _sa_params(*params)
    sg = SplitAttnGrads(*[_ptr(t) for t in grads])
    gws = torch.empty(int(lib.usseg_splitattn_mlp_bwd_ws_floats(C.byref(d))), dtype=torch.float32, device=dev)
    # sum_pixels dout*y per (image, channel) as per-workgroup rows, summed by the MLP kernel itself (no finishing launch between the two)
    L.check(lib.usseg_splitattn_bwd_fused(C.byref(d), y.data_ptr(), dout.data_ptr(), lddo, g[0].data_ptr(), g[1], g[2], C.byref(sp), s.data_ptr(),
                                          ws.data_ptr(), dg.data_ptr(), C.byref(sg), reduce_ws(dev).data_ptr(), gws.data_ptr(), _stream()),
            "splitattn_bwd_fused")
    if dy is None:
        assert d.R == 1, "the fused re-weighting backward needs identical radix branches (R == 1)"
        return s, dg
    L.check(lib.usseg_splitattn_apply_bwd_dy(C.byref(d), dout.data_ptr(), lddo, s.data_ptr(), dg.data_ptr(), dy.data_ptr(), geom(dy)[4],
                                             _stream()), "splitattn_apply_bwd_dy")
    return dy


# ------------------------------------------------------------------------------------------------ head softmax + loss
def class_loss(w, gamma=0.0, factor=1.0) -> L.ClassLoss:
    """A ``UssegClassLoss`` (usseg.h): l = -factor * sum_c w[c] * y_smoothed[c] * (1 - p[c])^gamma * log p[c] on clipped, un-normalised
    probabilities - VisionTransformer.my_loss_cat (factor 3, w = class_factor, gamma 0) and its focal line (factor 1, w = 1, gamma = alpha).
    ValueError for what the library would refuse: more than 8 weights, a gamma that is neither 0 nor in [1, 8], a negative or non-finite number."""
    w = [float(v) for v in w]
    gamma, factor = float(gamma), float(factor)
    if not 1 <= len(w) <= 8:
        raise ValueError(f"class loss: 1 to 8 class weights, got {len(w)}")
    if not (gamma == 0.0 or 1.0 <= gamma <= 8.0):
        raise ValueError(f"class loss: gamma must be 0 or lie in [1, 8], got {gamma}")
    if not all(math.isfinite(v) and v >= 0.0 for v in w + [factor]):
        raise ValueError(f"class loss: weights and factor must be finite and >= 0, got {w}, {factor}")
    return L.ClassLoss((L.c_f32 * 8)(*w), gamma, factor)


def softmax_loss(logits, y_true, probs, loss, dlogits, *, HW, C_classes, loss_kind=0, label_smoothing=0.1, clip_eps=1e-7,
                 inv_global_batch=1.0, scale=None, quad_w=0, class_loss=None):
    """logits fp32 [..., ldl]; y_true fp32 [..., C] or None; probs fp32 [..., C]; dlogits bf16 [..., 8] or None.
    ``quad_w`` = full-resolution width when logits / dlogits are in the head's space-to-depth layout [B,H/2,W/2,16].
    ``class_loss`` (``ops.class_loss(...)``): the loss is loss_kind 2, the scalar form of that class loss, instead of ``loss_kind``."""
    M = probs.numel() // C_classes
    ldl = logits.shape[-1]
    if class_loss is not None:
        assert scale is None and (loss is None or loss.numel() >= ACC_FLOATS)
        d = LossDesc(M, HW, C_classes, ldl, 16 if quad_w else 8, 2, label_smoothing, clip_eps, inv_global_batch, quad_w)
        L.check(L.load().usseg_softmax_loss_fwd_bwd_cl(C.byref(d), C.byref(class_loss), logits.data_ptr(), _ptr(y_true), probs.data_ptr(), _ptr(loss),
                                                       _ptr(dlogits), _stream()), "softmax_loss_cl")
        return
    assert loss is None or loss_kind == 1 or loss.numel() >= ACC_FLOATS, "the scalar loss accumulates through a USSEG_ACC_FLOATS buffer"
    d = LossDesc(M, HW, C_classes, ldl, 16 if quad_w else 8, loss_kind, label_smoothing, clip_eps, inv_global_batch, quad_w)
    L.check(L.load().usseg_softmax_loss_fwd_bwd(C.byref(d), logits.data_ptr(), _ptr(y_true), _ptr(scale), probs.data_ptr(), _ptr(loss),
                                                _ptr(dlogits), _stream()), "softmax_loss")


def head_quad_softmax_loss(x, wq, bias, C_classes, y_true, probs, loss, dlogits, *, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0,
                           class_loss=None) -> bool:
    """The quad-form head conv + softmax + loss (loss_kind 0, or the class loss ``class_loss``) in one launch; x [B,h,w,Cin_phys] bf16,
    wq [16][9*Cin_phys], probs [B,2h,2w,C] fp32,
    dlogits bf16 [B,h,w,16] or None.  False - nothing launched - when there is no fused kernel for the size (ordered-sum slots, LDS)."""
    B, h, w, Cx, ldx = geom(x)
    assert tuple(wq.shape) == (16, 9 * Cx) and (loss is None or loss.numel() >= ACC_FLOATS)
    if class_loss is not None:
        rc = L.load().usseg_head_quad_softmax_loss_cl(x.data_ptr(), B, h, w, Cx, ldx, wq.data_ptr(), bias.data_ptr(), C_classes, _ptr(y_true),
                                                      probs.data_ptr(), _ptr(loss), _ptr(dlogits), label_smoothing, clip_eps, inv_global_batch,
                                                      C.byref(class_loss), _stream())
    else:
        rc = L.load().usseg_head_quad_softmax_loss(x.data_ptr(), B, h, w, Cx, ldx, wq.data_ptr(), bias.data_ptr(), C_classes, _ptr(y_true), probs.data_ptr(),
                                                   _ptr(loss), _ptr(dlogits), label_smoothing, clip_eps, inv_global_batch, _stream())
    if rc == -2:
        return False
    L.check(rc, "head_quad_softmax_loss")
    return True


def loss_from_probs(probs, y_true, loss, *, HW, C_classes, loss_kind=0, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0, scale=None,
                    class_loss=None, as_map=False):
    """The reference's public loss methods on PROBABILITIES (compute_loss / my_loss_cat); ``loss`` (pre-zeroed) accumulates.
    ``class_loss``: that class loss (loss_kind 2) instead - the scalar in ``loss[0]``, or with ``as_map`` the [HW] map summed over the batch
    (VisionTransformer.my_loss_cat's return value; ``inv_global_batch`` is not applied to it)."""
    assert probs.dtype == torch.float32 and y_true.dtype == torch.float32 and probs.is_contiguous() and y_true.is_contiguous()
    M = probs.numel() // C_classes
    if class_loss is not None:
        assert scale is None and loss.numel() >= (HW if as_map else ACC_FLOATS)
        d = LossDesc(M, HW, C_classes, C_classes, 8, 2, label_smoothing, clip_eps, inv_global_batch, 0)
        L.check(L.load().usseg_loss_from_probs_cl(C.byref(d), C.byref(class_loss), probs.data_ptr(), y_true.data_ptr(), loss.data_ptr(), int(as_map),
                                                  _stream()), "loss_from_probs_cl")
        return
    assert loss_kind == 1 or loss.numel() >= ACC_FLOATS
    d = LossDesc(M, HW, C_classes, C_classes, 8, loss_kind, label_smoothing, clip_eps, inv_global_batch, 0)
    L.check(L.load().usseg_loss_from_probs(C.byref(d), probs.data_ptr(), y_true.data_ptr(), _ptr(scale), loss.data_ptr(), _stream()),
            "loss_from_probs")


# ------------------------------------------------------------------------------------------------ soft Dice / Tversky (+ CCE)
OVERLAP_ACC_FLOATS = L.OVERLAP_ACC_FLOATS   # [0] loss, [1] ticket, [2] CCE sum, [4..12) A_c, B_c, [16..32) I, P, Y, T, [32 + 16*b + k] partials
OVERLAP_KEYS = ("alpha", "beta", "smooth", "power", "class_weight", "ce_weight", "ov_weight")


def overlap_loss(class_weight, alpha=0.5, beta=0.5, smooth=1.0, power=1.0, ov_weight=1.0, ce_weight=0.0) -> L.OverlapLoss:
    """A ``UssegOverlapLoss`` (usseg.h): loss = ce_weight * CCE + ov_weight * ov_scale * sum_c w[c] * (1 - T_c)^power with the Tversky index
    T_c = (I_c + s) / ((1-a-b)*I_c + a*P_c + b*Y_c + s); alpha = beta = 0.5 is soft Dice.  ValueError for what the library would refuse:
    more than 4 weights, a power outside [1, 4], smooth <= 0, a negative or non-finite number - and for a loss with both weights zero."""
    w = [float(v) for v in class_weight]
    alpha, beta, smooth, power, ov_weight, ce_weight = (float(v) for v in (alpha, beta, smooth, power, ov_weight, ce_weight))
    if not 1 <= len(w) <= 4:
        raise ValueError(f"overlap loss: 1 to 4 class weights, got {len(w)}")
    if not 1.0 <= power <= 4.0:
        raise ValueError(f"overlap loss: power must lie in [1, 4], got {power}")
    if not (math.isfinite(smooth) and smooth > 0.0):
        raise ValueError(f"overlap loss: smooth must be finite and > 0, got {smooth}")
    if not all(math.isfinite(v) and v >= 0.0 for v in w + [alpha, beta, ov_weight, ce_weight]):
        raise ValueError(f"overlap loss: weights, alpha and beta must be finite and >= 0, got {w}, {alpha}, {beta}, {ov_weight}, {ce_weight}")
    if ov_weight == 0.0 and ce_weight == 0.0:
        raise ValueError("overlap loss: ov_weight and ce_weight are both zero")
    return L.OverlapLoss((L.c_f32 * 8)(*w), alpha, beta, smooth, power, ov_weight, ce_weight)


def overlap_loss_grid(M: int) -> int:
    """Workgroups of the sums pass for M pixels (usseg.h: the grid rule its rounding-error bound follows from)."""
    return int(L.load().usseg_overlap_loss_grid(int(M)))


def _overlap_desc(probs, y_true, HW, C_classes, lddl, label_smoothing, clip_eps, inv_global_batch, quad_w):
    assert probs.dtype == torch.float32 and y_true.dtype == torch.float32 and probs.is_contiguous() and y_true.is_contiguous()
    assert probs.shape == y_true.shape
    return LossDesc(probs.numel() // C_classes, HW, C_classes, C_classes, lddl, 0, label_smoothing, clip_eps, inv_global_batch, quad_w)


def overlap_loss_sums(probs, y_true, acc, *, overlap, HW, C_classes, ov_scale=1.0, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0):
    """Pass 1 on PROBABILITIES fp32 [..., C]: ``acc`` (fp32 [OVERLAP_ACC_FLOATS], zeroed once at allocation) receives the scalar loss in [0],
    the backward coefficients in [4..12) and the totals I, P, Y, T per class from [16], all bitwise reproducible."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 8, label_smoothing, clip_eps, inv_global_batch, 0)
    L.check(L.load().usseg_overlap_loss_sums(C.byref(d), C.byref(overlap), ov_scale, probs.data_ptr(), y_true.data_ptr(), acc.data_ptr(), acc.numel(),
                                             _stream()), "overlap_loss_sums")


def overlap_loss_bwd(probs, y_true, acc, dlogits, *, overlap, HW, C_classes, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0, quad_w=0):
    """Pass 2: d loss / d logits (bf16 [..., 8], or [B,H/2,W/2,16] with ``quad_w`` = the full-resolution width) from the probabilities, the labels and
    the coefficients ``overlap_loss_sums`` left in ``acc``."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 16 if quad_w else 8, label_smoothing, clip_eps, inv_global_batch, quad_w)
    L.check(L.load().usseg_overlap_loss_bwd(C.byref(d), C.byref(overlap), probs.data_ptr(), y_true.data_ptr(), acc.data_ptr(), acc.numel(),
                                            dlogits.data_ptr(), _stream()), "overlap_loss_bwd")


# ------------------------------------------------------------------------------------------------ distance maps, the boundary term
BOUNDARY_KEYS = ("weight", "class_weight", "threshold")


def boundary_loss(class_weight) -> L.BoundaryLoss:
    """A ``UssegBoundaryLoss`` (usseg.h): the per-class weights u[c] of L_B = wb * ov_scale / M * sum_m sum_c u[c] * p_c * phi_c.  ValueError for
    what the library would refuse."""
    u = [float(v) for v in class_weight]
    if not 1 <= len(u) <= 4:
        raise ValueError(f"boundary loss: 1 to 4 class weights, got {len(u)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in u):
        raise ValueError(f"boundary loss: class weights must be finite and >= 0, got {u}")
    return L.BoundaryLoss((L.c_f32 * 8)(*u))


def sdf_ws_bytes(B: int, H: int, W: int, C_classes: int) -> int:
    """Workspace bytes of ``sdf_labels`` (usseg_sdf_ws_bytes); ValueError for a shape the transform refuses."""
    n = int(L.load().usseg_sdf_ws_bytes(B, H, W, C_classes))
    if n < 0:
        raise ValueError(f"sdf_labels: H and W must lie in [1, 8192] and C in [1, 4], got {B}x{H}x{W}x{C_classes}")
    return n


def sdf_labels(y_true, phi=None, ws=None, *, threshold=0.5):
    """Kervadec's signed distance map of the labels (usseg.h usseg_sdf_labels): y_true fp32 [B,H,W,C] -> phi fp32 [B,H,W,C], exact.  ``phi`` and
    ``ws`` (uint8, ``sdf_ws_bytes`` long) are allocated when not given; a captured step passes its own."""
    assert y_true.dtype == torch.float32 and y_true.is_contiguous() and y_true.dim() == 4
    B, H, W, Cc = y_true.shape
    need = sdf_ws_bytes(B, H, W, Cc)
    if phi is None:
        phi = torch.empty_like(y_true)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=y_true.device)
    assert phi.dtype == torch.float32 and phi.is_contiguous() and phi.shape == y_true.shape and ws.dtype == torch.uint8
    L.check(L.load().usseg_sdf_labels(y_true.data_ptr(), B, H, W, Cc, float(threshold), phi.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdf_labels")
    return phi


def surface_dist(a, b, ws=None):
    """Surface-to-surface distances of two uint8 [N,H,W] masks (usseg.h usseg_surface_dist) -> (counters int64 [N,4], sums fp64 [N,2])."""
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous() and a.dim() == 3 and a.shape == b.shape
    N, H, W = a.shape
    need = int(L.load().usseg_surface_ws_bytes(N, H, W))
    if need < 0:
        raise ValueError(f"surface_dist: H and W must lie in [1, 8192], got {N}x{H}x{W}")
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=a.device)
    counters = torch.empty((N, 4), dtype=torch.int64, device=a.device)
    sums = torch.empty((N, 2), dtype=torch.float64, device=a.device)
    L.check(L.load().usseg_surface_dist(a.data_ptr(), b.data_ptr(), N, H, W, counters.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "surface_dist")
    return counters, sums


def surface_stats_ws_bytes(N: int, H: int, W: int) -> int:
    """Workspace bytes of ``surface_stats`` (usseg_surface_stats_ws_bytes); ValueError for a shape it refuses."""
    n = int(L.load().usseg_surface_stats_ws_bytes(N, H, W))
    if n < 0:
        raise ValueError(f"surface_stats: H and W must lie in [1, 8192], got {N}x{H}x{W}")
    return n


def surface_stats(a, b, percentiles=(), tol2=(), *, ws=None, out=None):
    """``surface_dist`` plus the order statistics and tolerance counts behind HD95 and the surface Dice (usseg.h usseg_surface_stats): two
    uint8 [N,H,W] masks, up to 4 ``percentiles`` q in [0, 100] (passed on as the fp64 quantile q / 100) and up to 4 squared tolerances
    ``tol2`` (ints >= 0) -> (counters int64 [N,4], sums fp64 [N,2], sel int32 [N,3,P,2], within int64 [N,T,2]).  ``ws`` (uint8,
    ``surface_stats_ws_bytes`` long) and ``out`` (those four tensors) are allocated when not given; a captured region passes its own."""
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous() and a.dim() == 3 and a.shape == b.shape
    N, H, W = a.shape
    quant = [float(q) / 100 for q in percentiles]
    t2 = [int(t) for t in tol2]
    P, T = len(quant), len(t2)
    if P > 4 or T > 4:
        raise ValueError(f"surface_stats: at most 4 percentiles and 4 tolerances, got {P} and {T}")
    if not all(math.isfinite(q) and 0.0 <= q <= 1.0 for q in quant):
        raise ValueError(f"surface_stats: percentiles must lie in [0, 100], got {list(percentiles)}")
    if not all(0 <= t < 2 ** 31 and t == v for t, v in zip(t2, tol2)):
        raise ValueError(f"surface_stats: squared tolerances must be integers in [0, 2^31), got {list(tol2)}")
    need = surface_stats_ws_bytes(N, H, W)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=a.device)
    if out is None:
        out = (torch.empty((N, 4), dtype=torch.int64, device=a.device), torch.empty((N, 2), dtype=torch.float64, device=a.device),
               torch.empty((N, 3, P, 2), dtype=torch.int32, device=a.device), torch.empty((N, T, 2), dtype=torch.int64, device=a.device))
    counters, sums, sel, within = out
    for t, dt, shape in ((counters, torch.int64, (N, 4)), (sums, torch.float64, (N, 2)), (sel, torch.int32, (N, 3, P, 2)), (within, torch.int64, (N, T, 2))):
        assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == a.device and ws.dtype == torch.uint8
    if N == 0:                                          # (empty tensors have no address to pass; the library launches nothing for N == 0 either)
        return counters, sums, sel, within
    L.check(L.load().usseg_surface_stats(a.data_ptr(), b.data_ptr(), N, H, W, (C.c_double * max(P, 1))(*quant), P, (C.c_int32 * max(T, 1))(*t2), T,
                                         counters.data_ptr(), sums.data_ptr(), sel.data_ptr() if P else None, within.data_ptr() if T else None,
                                         ws.data_ptr(), ws.numel(), _stream()), "surface_stats")
    return counters, sums, sel, within


# ---- connected components (csrc/components.hip) -------------------------------------------------------------------------------------------
COMPONENT_STAT_FIELDS = ("area", "y_min", "x_min", "y_max", "x_max", "sum_y", "sum_x", "peak_bits")


def components_ws_bytes(N: int, H: int, W: int) -> int:
    """Workspace bytes of ``label_components`` and ``clean_mask`` (usseg_components_ws_bytes); ValueError for a refused shape."""
    n = int(L.load().usseg_components_ws_bytes(N, H, W))
    if n < 0:
        raise ValueError(f"components: H and W must lie in [1, 8192], N in [0, 65535] and N*H*W <= 2^29, got {N}x{H}x{W}")
    return n


def _component_mask(mask, what):
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 3, f"{what}: a contiguous uint8 [N,H,W] mask"
    return mask.shape


def _component_ws(ws, need, device):
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    return ws


def label_components(mask, connectivity=8, labels=None, count=None, ws=None):
    """Connected components of a uint8 [N,H,W] mask (usseg.h usseg_label_components) -> (labels int32 [N,H,W], count int32 [N]): 0 outside,
    1..K_n inside in ``scipy.ndimage.label``'s numbering.  ``labels``, ``count`` and ``ws`` (uint8, ``components_ws_bytes`` long) are
    allocated when not given."""
    N, H, W = _component_mask(mask, "label_components")
    ws = _component_ws(ws, components_ws_bytes(N, H, W), mask.device)
    if labels is None:
        labels = torch.empty((N, H, W), dtype=torch.int32, device=mask.device)
    if count is None:
        count = torch.empty((max(N, 1),), dtype=torch.int32, device=mask.device)[:N]
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape == mask.shape
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == N
    if N == 0:
        return labels, count
    L.check(L.load().usseg_label_components(mask.data_ptr(), N, H, W, int(connectivity), labels.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream()), "label_components")
    return labels, count


def component_stats(labels, cap, prob=None):
    """Per-component table of a label image (usseg.h usseg_component_stats) -> int64 [N,cap,8], the fields of ``COMPONENT_STAT_FIELDS``."""
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.dim() == 3
    N, H, W = labels.shape
    cap = int(cap)
    if cap < 0:
        raise ValueError(f"component_stats: cap must be >= 0, got {cap}")
    if prob is not None:
        assert prob.dtype == torch.float32 and prob.is_contiguous() and prob.shape == labels.shape
    stats = torch.empty((N, cap, 8), dtype=torch.int64, device=labels.device)
    if N * cap:
        L.check(L.load().usseg_component_stats(labels.data_ptr(), prob.data_ptr() if prob is not None else None, N, H, W, cap, stats.data_ptr(), _stream()),
                "component_stats")
    return stats


def clean_mask(mask, prob=None, *, connectivity=8, min_area=1, min_peak=0.0, out=None, ws=None):
    """uint8 [N,H,W]: 1 on the components of ``mask`` with at least ``min_area`` pixels and (with ``prob``) a peak of at least ``min_peak``
    (usseg.h usseg_clean_mask).  ``out`` may be ``mask``; no host synchronisation, so the call can be captured in a graph."""
    N, H, W = _component_mask(mask, "clean_mask")
    ws = _component_ws(ws, components_ws_bytes(N, H, W), mask.device)
    if out is None:
        out = torch.empty_like(mask)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == mask.shape
    if prob is not None:
        assert prob.dtype == torch.float32 and prob.is_contiguous() and prob.shape == mask.shape
    if N == 0:
        return out
    L.check(L.load().usseg_clean_mask(mask.data_ptr(), prob.data_ptr() if prob is not None else None, N, H, W, int(connectivity), int(min_area),
                                      float(min_peak), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "clean_mask")
    return out


def component_overlap(la, lb, cap_a, cap_b):
    """Pixels of each component of ``la`` inside any component of ``lb`` and the reverse (usseg.h usseg_component_overlap)
    -> (hit_a int32 [N,cap_a], hit_b int32 [N,cap_b])."""
    assert la.dtype == torch.int32 and lb.dtype == torch.int32 and la.is_contiguous() and lb.is_contiguous() and la.dim() == 3 and la.shape == lb.shape
    N, H, W = la.shape
    cap_a, cap_b = int(cap_a), int(cap_b)
    if cap_a < 0 or cap_b < 0:
        raise ValueError(f"component_overlap: caps must be >= 0, got {cap_a} and {cap_b}")
    hit_a = torch.empty((N, cap_a), dtype=torch.int32, device=la.device)
    hit_b = torch.empty((N, cap_b), dtype=torch.int32, device=la.device)
    if N and (cap_a or cap_b):
        L.check(L.load().usseg_component_overlap(la.data_ptr(), lb.data_ptr(), N, H, W, cap_a, cap_b, hit_a.data_ptr() if cap_a else None,
                                                 hit_b.data_ptr() if cap_b else None, _stream()), "component_overlap")
    return hit_a, hit_b


# ---- per-image scores in pixels and physical units (csrc/scores.hip, include/usseg_scores.h) -----------------------------------------------
COMPONENT_MEASURE_FIELDS = ("pixels", "sum_w", "sum_wx", "sum_wy", "xq_min", "xq_max", "yq_min", "yq_max")


def _scores_out(out, shape, device, what):
    if out is None:
        return torch.empty(shape, dtype=torch.int64, device=device)
    assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == tuple(shape) and out.device == device, \
        f"{what}: a contiguous int64 {tuple(shape)} on {device}"
    return out


def _scores_grid(t, shape, dtype, what):
    assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.is_cuda, f"{what}: a contiguous {dtype} {tuple(shape)} on the GPU"
    return t


def image_confusion(pred, truth, num_classes=2, weight=None, *, out=None):
    """The confusion table of every image (usseg_scores.h usseg_image_confusion): ``pred``, ``truth`` uint8 [N,H,W] class ids on the GPU,
    ``weight`` uint32-valued [H,W] (an int32 or uint32 tensor, e.g. ``ScanGeometry.wq``) or None -> (cm int64 [N,C,C] with cm[n][truth][pred],
    wcm int64 [N,C,C] or None, invalid int64 [N]).  ``out`` = (cm, wcm, invalid) buffers to write into (wcm None without a weight)."""
    N, H, W = _component_mask(pred, "image_confusion")
    assert pred.is_cuda, "image_confusion runs on the GPU only"
    _scores_grid(truth, (N, H, W), torch.uint8, "image_confusion: truth")
    C_ = int(num_classes)
    if not 2 <= C_ <= 4:
        raise ValueError(f"image_confusion: num_classes must lie in [2, 4], got {num_classes}")
    if weight is not None:
        assert weight.dtype in (torch.int32, torch.uint32), "image_confusion: weight must be a 32-bit integer tensor"
        _scores_grid(weight, (H, W), weight.dtype, "image_confusion: weight")
    cm, wcm, invalid = out if out is not None else (None, None, None)
    if (wcm is not None) != (weight is not None) and out is not None:
        raise ValueError("image_confusion: the wcm buffer goes with a weight: both or neither")
    cm = _scores_out(cm, (N, C_, C_), pred.device, "image_confusion: cm")
    wcm = _scores_out(wcm, (N, C_, C_), pred.device, "image_confusion: wcm") if weight is not None else None
    invalid = _scores_out(invalid, (N,), pred.device, "image_confusion: invalid")
    if N:
        L.check(L.load().usseg_image_confusion(pred.data_ptr(), truth.data_ptr(), weight.data_ptr() if weight is not None else None, N, H, W, C_,
                                               cm.data_ptr(), wcm.data_ptr() if wcm is not None else None, invalid.data_ptr(), _stream()), "image_confusion")
    return cm, wcm, invalid


def component_measure(labels, weight, xq, yq, cap, *, out=None):
    """Size, position and extent of every component in fixed-point physical units (usseg_scores.h usseg_component_measure): ``labels`` the
    int32 [N,H,W] of ``label_components``, ``weight`` / ``xq`` / ``yq`` the [H,W] tables of ``metrics.ScanGeometry`` on the GPU
    -> int64 [N,cap,8], the fields of ``COMPONENT_MEASURE_FIELDS``; absent ids: zeros and the extents (SCORES_EMPTY_MIN, -1)."""
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.dim() == 3 and labels.is_cuda, "component_measure: contiguous int32 [N,H,W] labels on the GPU"
    N, H, W = labels.shape
    cap = int(cap)
    if cap < 0:
        raise ValueError(f"component_measure: cap must be >= 0, got {cap}")
    assert weight.dtype in (torch.int32, torch.uint32), "component_measure: weight must be a 32-bit integer tensor"
    _scores_grid(weight, (H, W), weight.dtype, "component_measure: weight")
    _scores_grid(xq, (H, W), torch.int32, "component_measure: xq")
    _scores_grid(yq, (H, W), torch.int32, "component_measure: yq")
    out = _scores_out(out, (N, cap, 8), labels.device, "component_measure: out")
    if N * cap:
        L.check(L.load().usseg_component_measure(labels.data_ptr(), weight.data_ptr(), xq.data_ptr(), yq.data_ptr(), N, H, W, cap, out.data_ptr(), _stream()),
                "component_measure")
    return out


def bootstrap_check_rows(rows_max_abs: int, U: int) -> None:
    """The overflow rule of ``bootstrap_sums``: U draws of values up to ``rows_max_abs`` must stay inside int64, |v| <= 2^62 / U."""
    if U > 0 and int(rows_max_abs) > (1 << 62) // int(U):
        raise ValueError(f"bootstrap_sums: a value of magnitude {int(rows_max_abs)} times {U} draws can overflow int64 (|v| <= 2^62 / U)")


def bootstrap_sums(rows, replicates, seed=0, *, out=None, check=True):
    """Bootstrap replicates of the column sums of ``rows`` int64 [U,K] on the GPU (usseg_scores.h usseg_bootstrap_sums) -> int64 [R,K]; the
    draws are the header's counter-based generator, so (seed, r, U) fix replicate r.  ``check`` reads the largest magnitude back once to
    refuse rows with |v| > 2^62 / U; pass ``check=False`` (after ``bootstrap_check_rows`` on the host) inside a graph capture."""
    assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.dim() == 2 and rows.is_cuda, "bootstrap_sums: contiguous int64 [U,K] rows on the GPU"
    U, K = rows.shape
    R, seed = int(replicates), int(seed)
    if not 1 <= K <= L.SCORES_BOOT_MAX_K:
        raise ValueError(f"bootstrap_sums: K must lie in [1, {L.SCORES_BOOT_MAX_K}], got {K}")
    if not 0 <= R <= L.SCORES_BOOT_MAX or U > L.SCORES_BOOT_MAX:
        raise ValueError(f"bootstrap_sums: R and U must not exceed 2^20, got R = {R}, U = {U}")
    if R > 0 and U == 0:
        raise ValueError(f"bootstrap_sums: {R} replicates of an empty table")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"bootstrap_sums: the seed must fit 64 unsigned bits, got {seed}")
    if check and U:
        lo, hi = torch.aminmax(rows)
        bootstrap_check_rows(max(-int(lo), int(hi)), U)
    out = _scores_out(out, (R, K), rows.device, "bootstrap_sums: out")
    if R and U:
        L.check(L.load().usseg_bootstrap_sums(rows.data_ptr(), U, K, seed, R, out.data_ptr(), _stream()), "bootstrap_sums")
    return out


def overlap_boundary_loss_sums(probs, y_true, phi, acc, *, overlap, boundary, wb, HW, C_classes, ov_scale=1.0, label_smoothing=0.1, clip_eps=1e-7,
                               inv_global_batch=1.0):
    """``overlap_loss_sums`` plus the boundary term: ``phi`` = ``sdf_labels(y_true)``, ``boundary`` a ``boundary_loss(...)``, ``wb`` a DEVICE fp32
    tensor holding the boundary weight (read when the kernel runs).  acc[0] = overlap loss + L_B, acc[12] = L_B, acc[13] = wb*ov_scale/M."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 8, label_smoothing, clip_eps, inv_global_batch, 0)
    assert phi.dtype == torch.float32 and phi.is_contiguous() and phi.shape == probs.shape and wb.dtype == torch.float32 and wb.device == probs.device
    L.check(L.load().usseg_overlap_boundary_loss_sums(C.byref(d), C.byref(overlap), ov_scale, probs.data_ptr(), y_true.data_ptr(), phi.data_ptr(),
                                                      C.byref(boundary), wb.data_ptr(), acc.data_ptr(), acc.numel(), _stream()),
            "overlap_boundary_loss_sums")


def overlap_boundary_loss_bwd(probs, y_true, phi, acc, dlogits, *, overlap, boundary, HW, C_classes, label_smoothing=0.1, clip_eps=1e-7,
                              inv_global_batch=1.0, quad_w=0):
    """``overlap_loss_bwd`` with the boundary summand acc[13]*u[c]*phi_c(m) in G_c(m): one bf16 rounding."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 16 if quad_w else 8, label_smoothing, clip_eps, inv_global_batch, quad_w)
    assert phi.dtype == torch.float32 and phi.is_contiguous() and phi.shape == probs.shape
    L.check(L.load().usseg_overlap_boundary_loss_bwd(C.byref(d), C.byref(overlap), probs.data_ptr(), y_true.data_ptr(), phi.data_ptr(), C.byref(boundary),
                                                     acc.data_ptr(), acc.numel(), dlogits.data_ptr(), _stream()), "overlap_boundary_loss_bwd")


# ------------------------------------------------------------------------------------------------ stable radix sort, the Lovasz-softmax loss
SORT_TILE, SORT_DIGIT_BITS = L.SORT_TILE, L.SORT_DIGIT_BITS
LOVASZ_KEYS = ("classes", "class_weight", "lv_weight", "ce_weight", "threshold")
_WORDS = (torch.int32, getattr(torch, "uint32", torch.int32))


def sort_ws_bytes(S: int, n: int) -> int:
    need = int(L.load().usseg_sort_ws_bytes(int(S), int(n)))
    if need < 0:
        raise ValueError(f"sort_pairs: at most 65535 segments of at most 2^29 pairs, got {S} x {n}")
    return need


def sort_pairs(keys, vals, key_bits=32, ws=None):
    """A stable ascending sort of 32-bit (key, value) pairs on the low ``key_bits`` bits of the key, read as unsigned (usseg.h
    usseg_sort_pairs_u32): ``keys`` and ``vals`` [S, n] (or [n]: one segment), int32 or uint32 -> (sorted keys, their values), each row on its own.
    ``ws`` (uint8, ``sort_ws_bytes(S, n)`` long) is allocated when not given; a captured step passes its own."""
    assert keys.dtype in _WORDS and vals.dtype in _WORDS and keys.is_contiguous() and vals.is_contiguous() and keys.shape == vals.shape
    assert keys.dim() in (1, 2)
    S, n = (1, keys.shape[0]) if keys.dim() == 1 else keys.shape
    if not 1 <= int(key_bits) <= 32:
        raise ValueError(f"sort_pairs: key_bits must lie in [1, 32], got {key_bits}")
    need = sort_ws_bytes(S, n)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=keys.device)
    assert ws.dtype == torch.uint8
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    if S and n:
        L.check(L.load().usseg_sort_pairs_u32(keys.data_ptr(), vals.data_ptr(), S, n, int(key_bits), ko.data_ptr(), vo.data_ptr(), ws.data_ptr(),
                                              ws.numel(), _stream()), "sort_pairs")
    return ko, vo


def lovasz_loss(class_weight, lv_weight=1.0, ce_weight=0.0, threshold=0.5, classes="present") -> L.LovaszLoss:
    """A ``UssegLovaszLoss`` (usseg.h): loss = ce_weight * CCE + lv_weight * ov_scale * mean over the classes of ``classes`` ("present": those
    with a foreground pixel in the call; "all") of w[c] * the Lovasz extension of the Jaccard loss of class c.  ValueError for what the library
    would refuse: more than 4 weights, a negative or non-finite number, an unknown ``classes`` - and for a loss with both weights zero."""
    w = [float(v) for v in class_weight]
    lv_weight, ce_weight, threshold = float(lv_weight), float(ce_weight), float(threshold)
    if not 1 <= len(w) <= 4:
        raise ValueError(f"lovasz loss: 1 to 4 class weights, got {len(w)}")
    if classes not in ("present", "all"):
        raise ValueError(f"lovasz loss: classes must be 'present' or 'all', got {classes!r}")
    if not all(math.isfinite(v) and v >= 0.0 for v in w + [lv_weight, ce_weight]):
        raise ValueError(f"lovasz loss: weights must be finite and >= 0, got {w}, {lv_weight}, {ce_weight}")
    if not math.isfinite(threshold):
        raise ValueError(f"lovasz loss: threshold must be finite, got {threshold}")
    if lv_weight == 0.0 and ce_weight == 0.0:
        raise ValueError("lovasz loss: lv_weight and ce_weight are both zero")
    return L.LovaszLoss((L.c_f32 * 8)(*w), lv_weight, ce_weight, threshold, 1 if classes == "all" else 0)


def lovasz_ws_bytes(M: int, C_classes: int) -> int:
    need = int(L.load().usseg_lovasz_ws_bytes(int(M), int(C_classes)))
    if need < 0:
        raise ValueError(f"lovasz loss: at most 2^29 pixels of 1 to 4 classes, got {M} x {C_classes}")
    return need


def lovasz_coeffs(probs, y_true, g, counts, ws, *, lovasz, HW, C_classes):
    """The Lovasz gradient of every pixel and class: ``g`` fp32 (the shape of ``probs``) and ``counts`` int32 [C] = the foreground pixels per class,
    through the device sort.  ``ws``: uint8, ``lovasz_ws_bytes(M, C)`` long.  Sixteen launches whatever the data."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 8, 0.1, 1e-7, 1.0, 0)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == probs.shape and counts.dtype == torch.int32 and counts.numel() >= C_classes
    assert ws.dtype == torch.uint8
    L.check(L.load().usseg_lovasz_coeffs(C.byref(d), lovasz, probs.data_ptr(), y_true.data_ptr(), g.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream()), "lovasz_coeffs")


def lovasz_loss_sums(probs, y_true, g, counts, acc, *, lovasz, HW, C_classes, ov_scale=1.0, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0):
    """``acc`` (fp32 [OVERLAP_ACC_FLOATS], zeroed once at allocation) receives the scalar loss in [0], the CCE pixel sum in [2], k_c in [4..8) and
    L_c from [16], all bitwise reproducible (the overlap sums pass's reduction and grid rule)."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 8, label_smoothing, clip_eps, inv_global_batch, 0)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == probs.shape and counts.dtype == torch.int32 and counts.numel() >= C_classes
    L.check(L.load().usseg_lovasz_loss_sums(C.byref(d), lovasz, ov_scale, probs.data_ptr(), y_true.data_ptr(), g.data_ptr(), counts.data_ptr(), acc.data_ptr(),
                                            acc.numel(), _stream()), "lovasz_loss_sums")


def lovasz_loss_bwd(probs, y_true, g, acc, dlogits, *, lovasz, HW, C_classes, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0, quad_w=0):
    """d loss / d logits (bf16 [..., 8], or [B,H/2,W/2,16] with ``quad_w``) from the probabilities, the labels, ``g`` and the k_c in ``acc``."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 16 if quad_w else 8, label_smoothing, clip_eps, inv_global_batch, quad_w)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == probs.shape
    L.check(L.load().usseg_lovasz_loss_bwd(C.byref(d), lovasz, probs.data_ptr(), y_true.data_ptr(), g.data_ptr(), acc.data_ptr(), acc.numel(),
                                           dlogits.data_ptr(), _stream()), "lovasz_loss_bwd")


# ------------------------------------------------------------------------------------------------ exact selection, the top-k cross-entropy
TOPK_KEYS = ("fraction", "scope", "tk_weight")
TOPK_SCOPES = ("batch", "image")


def topk_fraction_value(fraction) -> float:
    """The fraction as the device float holds it; ValueError unless it is finite and lies in (0, 1]."""
    f = float(fraction)
    if not (math.isfinite(f) and 0.0 < f <= 1.0):
        raise ValueError(f"topk: fraction must be finite and lie in (0, 1], got {fraction}")
    return f


def topk_loss(tk_weight=1.0, scope="batch") -> L.TopkLoss:
    """A ``UssegTopkLoss`` (usseg.h): tk_weight * the mean of the k = max(1, floor(fraction * n)) largest per-pixel cross-entropies of each
    segment - the call's pixels (``scope="batch"``) or each image (``"image"``).  The fraction is a device float the kernels read when they run.
    ValueError for what the library would refuse."""
    tk_weight = float(tk_weight)
    if scope not in TOPK_SCOPES:
        raise ValueError(f"topk: scope must be one of {TOPK_SCOPES}, got {scope!r}")
    if not (math.isfinite(tk_weight) and tk_weight >= 0.0):
        raise ValueError(f"topk: tk_weight must be finite and >= 0, got {tk_weight}")
    return L.TopkLoss(tk_weight, TOPK_SCOPES.index(scope))


def topk_select_ws_bytes(S: int) -> int:
    need = int(L.load().usseg_topk_select_ws_bytes(int(S)))
    if need < 0:
        raise ValueError(f"topk_select: at most 2^29 segments, got {S}")
    return need


def topk_select(keys, fraction=None, k=None, ws=None, sel=None):
    """The k-th largest key of every row of ``keys`` ([S, n] or [n]; int32 or uint32, read as unsigned), exactly (usseg.h usseg_topk_select)
    -> ``sel`` int32 [S, 4] = (t as its bits, keys above t, keys equal to t, k).  ``fraction``: a DEVICE fp32 tensor, read when the kernels run
    (k = max(1, min(n, floor(fraction * n)))) - or an explicit ``k``.  ``ws`` (uint8, ``topk_select_ws_bytes(S)`` long) and ``sel`` are
    allocated when not given; a captured region passes its own."""
    assert keys.dtype in _WORDS and keys.is_contiguous() and keys.dim() in (1, 2)
    S, n = (1, keys.shape[0]) if keys.dim() == 1 else keys.shape
    if (fraction is None) == (k is None):
        raise ValueError("topk_select: give the device fraction or an explicit k")
    if fraction is not None:
        assert fraction.dtype == torch.float32 and fraction.device == keys.device and fraction.numel() >= 1
    elif not 1 <= int(k) <= n:
        raise ValueError(f"topk_select: 1 <= k <= n = {n}, got {k}")
    need = topk_select_ws_bytes(S)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=keys.device)
    if sel is None:
        sel = torch.empty((S, 4), dtype=torch.int32, device=keys.device)
    assert ws.dtype == torch.uint8 and sel.dtype == torch.int32 and sel.is_contiguous() and tuple(sel.shape) == (S, 4)
    if S:
        L.check(L.load().usseg_topk_select(keys.data_ptr(), S, n, None if fraction is None else fraction.data_ptr(), 0 if k is None else int(k),
                                           sel.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "topk_select")
    return sel


def topk_ws_bytes(M: int, HW: int, scope="batch") -> int:
    need = int(L.load().usseg_topk_ws_bytes(int(M), int(HW), TOPK_SCOPES.index(scope)))
    if need < 0:
        raise ValueError(f"topk: at most 2^29 pixels, a multiple of HW, got {M} with HW = {HW}")
    return need


def topk_ws_views(ws, M: int, HW: int, scope="batch"):
    """The two results the top-k calls keep in their workspace -> (l fp32 [M], sel int32 [S, 4]) as views of ``ws`` (usseg.h has the layout)."""
    S = M // HW if scope == "image" else 1
    a = lambda b: (b + 255) // 256 * 256
    off = a(4 * M) + a(topk_select_ws_bytes(S))
    return ws[:4 * M].view(torch.float32), ws[off:off + 16 * S].view(torch.int32).view(S, 4)


def topk_pixel_loss(probs, y_true, fraction, ws, *, topk, HW, C_classes, label_smoothing=0.1, clip_eps=1e-7):
    """The per-pixel cross-entropy of every pixel and its exact selection into ``ws`` (uint8, ``topk_ws_bytes`` long; ``topk_ws_views`` reads
    them): five kernels and one memset whatever the data.  ``fraction``: a DEVICE fp32 tensor, read when the kernels run."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 8, label_smoothing, clip_eps, 1.0, 0)
    assert fraction.dtype == torch.float32 and fraction.device == probs.device and fraction.numel() >= 1 and ws.dtype == torch.uint8
    L.check(L.load().usseg_topk_pixel_loss(C.byref(d), topk, fraction.data_ptr(), probs.data_ptr(), y_true.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "topk_pixel_loss")


def topk_loss_sums(probs, ws, acc, *, topk, HW, C_classes, overlap_acc=None, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0):
    """``acc`` (fp32 [OVERLAP_ACC_FLOATS], zeroed once at allocation) receives the scalar loss in [0] (plus ``overlap_acc[0]`` when given), the plain
    CCE pixel sum in [2], the coefficient tk_weight * inv_global_batch * n / k in [4] and sum a*l in [5], all bitwise reproducible.  ``probs``
    gives the shape only."""
    d = LossDesc(probs.numel() // C_classes, HW, C_classes, C_classes, 8, 0, label_smoothing, clip_eps, inv_global_batch, 0)
    L.check(L.load().usseg_topk_loss_sums(C.byref(d), topk, ws.data_ptr(), ws.numel(), _ptr(overlap_acc), acc.data_ptr(), acc.numel(), _stream()),
            "topk_loss_sums")


def topk_loss_bwd(probs, y_true, ws, acc, dlogits, *, topk, HW, C_classes, overlap_acc=None, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0,
                  quad_w=0):
    """d loss / d logits (bf16 [..., 8], or [B,H/2,W/2,16] with ``quad_w``) from the probabilities, the labels, l and sel in ``ws`` and the
    coefficient in ``acc`` - plus the Dice term's A_c*y + B_c from ``overlap_acc`` when given."""
    d = _overlap_desc(probs, y_true, HW, C_classes, 16 if quad_w else 8, label_smoothing, clip_eps, inv_global_batch, quad_w)
    L.check(L.load().usseg_topk_loss_bwd(C.byref(d), topk, probs.data_ptr(), y_true.data_ptr(), ws.data_ptr(), ws.numel(), acc.data_ptr(), acc.numel(),
                                         _ptr(overlap_acc), dlogits.data_ptr(), _stream()), "topk_loss_bwd")


# ------------------------------------------------------------------------------------------------ knowledge distillation (usseg_distill.h)
DISTILL_ACC_FLOATS = L.DISTILL_ACC_FLOATS   # [0] loss, [1] ticket, [2] sum hard, [3] sum soft, [4] weighted hard term, [5] weighted soft term, partials
DISTILL_SETTINGS = L.DISTILL_SETTINGS       # the device table: [0] temperature, [1] soft_weight, [2] hard_weight, [3] reserved


def distill_grid(M: int) -> int:
    """Workgroups of the distillation launch for M pixels (usseg_distill.h: the grid rule the accumulator's size follows from)."""
    return int(L.load().usseg_distill_grid(int(M)))


def distill_loss(probs, y_true, q, settings, acc, dlogits=None, *, HW, C_classes, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=1.0, quad_w=0):
    """The distillation loss of usseg_distill.h in ONE launch: ``probs`` (the student's), ``y_true`` and ``q`` (the teacher's probabilities) fp32
    [..., C]; ``settings`` a DEVICE fp32 tensor [DISTILL_SETTINGS] = (temperature, soft_weight, hard_weight, 0), read when the kernel runs;
    ``acc`` fp32 [DISTILL_ACC_FLOATS], zeroed once at allocation: the scalar loss in [0], the hard and soft pixel sums in [2], [3], the two
    weighted terms in [4], [5], all bitwise reproducible.  ``dlogits`` (bf16 [..., 8], or [B,H/2,W/2,16] with ``quad_w`` = the full-resolution
    width) receives d loss / d logits, or None for the loss alone."""
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (probs, y_true, q)) and probs.shape == y_true.shape == q.shape
    assert settings.dtype == torch.float32 and settings.numel() >= DISTILL_SETTINGS and settings.device == probs.device and acc.dtype == torch.float32
    d = L.DistillDesc(probs.numel() // C_classes, HW, C_classes, 16 if quad_w else 8, quad_w, label_smoothing, clip_eps, inv_global_batch)
    L.check(L.load().usseg_distill_loss(C.byref(d), probs.data_ptr(), y_true.data_ptr(), q.data_ptr(), settings.data_ptr(), acc.data_ptr(), acc.numel(),
                                        _ptr(dlogits), _stream()), "distill_loss")


def quad_bias_expand(bias, C_logical, out):
    L.check(L.load().usseg_quad_bias_expand(bias.data_ptr(), C_logical, out.numel() // 4, out.data_ptr(), _stream()), "quad_bias_expand")


def space_to_depth2(full, quad, Np, to_quad=True):
    """full [B,2H,2W,C] (channel-slice views allowed) <-> quad [B,H,W,4*Np]: quad[b,i,j,(2a+b')*Np+n] = full[b,2i+a,2j+b',n]."""
    B, H2, W2, Cc, ldf = geom(full)
    _, H, W, _, ldq = geom(quad)
    assert (H2, W2) == (2 * H, 2 * W)
    L.check(L.load().usseg_space_to_depth2(full.data_ptr(), B, H, W, Cc, ldf, quad.data_ptr(), Np, ldq, 1 if to_quad else 0, _stream()),
            "space_to_depth2")


def tconv_quad_fwd(x, wq_f, bias_q, ksize, Np, y4):
    B, H, W, Cin, ldx = geom(x)
    d = _conv_desc(B, H, W, Cin, 4 * Np, ldx, geom(y4)[4], 3, 1)
    L.check(L.load().usseg_tconv_quad_fwd(C.byref(d), ksize, Np, x.data_ptr(), wq_f.data_ptr(), _ptr(bias_q), y4.data_ptr(), _stream()), "tconv_quad_fwd")
    return y4


def tconv_quad_dgrad(dy4, wq_d, ksize, Np, dx):
    B, H, W, _, ldy = geom(dy4)
    _, _, _, Cin, ldx = geom(dx)
    d = _conv_desc(B, H, W, Cin, 4 * Np, ldx, ldy, 3, 1)
    L.check(L.load().usseg_tconv_quad_dgrad(C.byref(d), ksize, Np, dy4.data_ptr(), wq_d.data_ptr(), dx.data_ptr(), _stream()), "tconv_quad_dgrad")
    return dx


def tconv_quad_wgrad(x, dy4, ksize, Np, dq):
    B, H, W, Cin, ldx = geom(x)
    d = _conv_desc(B, H, W, Cin, 4 * Np, ldx, geom(dy4)[4], 3, 1)
    ws = wgrad_ws(x.device)
    L.check(L.load().usseg_tconv_quad_wgrad(C.byref(d), ksize, Np, x.data_ptr(), dy4.data_ptr(), dq.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream()), "tconv_quad_wgrad")


def quad_bias_fold(d16, C_classes, dbias):
    L.check(L.load().usseg_quad_bias_fold(d16.data_ptr(), C_classes, dbias.data_ptr(), _stream()), "quad_bias_fold")


def tconv_quad_unpack(dq, Cin_phys, Cin, Cout, Np, ksize, grad):
    L.check(L.load().usseg_tconv_quad_unpack(dq.data_ptr(), Cin_phys, Cin, Cout, Np, ksize, grad.data_ptr(), _stream()), "tconv_quad_unpack")


def quad_head_fold(dq, Cin_phys, Cin, Cout, Np, ksize, grad, d16, dbias):
    """tconv_quad_unpack + quad_bias_fold in one launch (the tail of the quad-form head's backward)."""
    L.check(L.load().usseg_quad_head_fold(dq.data_ptr(), Cin_phys, Cin, Cout, Np, ksize, grad.data_ptr(), d16.data_ptr(), dbias.data_ptr(), _stream()),
            "quad_head_fold")


def loss_cat_scale(y_true, scale):
    B, H, W, Cc = y_true.shape
    L.check(L.load().usseg_loss_cat_scale(y_true.data_ptr(), B, H * W, Cc, scale.data_ptr(), _stream()), "loss_cat_scale")


# ------------------------------------------------------------------------------------------------ ViT attention helpers
def gemm_nt_batched(x, w, y, M, N, K, ldx, ldw, ldy, nb1, nb2, xs, ws, ys, out_f32=False):
    """Y[b1,b2][m][n] = sum_k X[b1,b2][m][k] W[b1,b2][n][k]; x/w/y are tensors whose data_ptr is the (0,0) batch base."""
    d = GemmDesc(M, N, K, ldx, ldw, ldy, nb1, nb2, xs[0], xs[1], ws[0], ws[1], ys[0], ys[1], OUT_F32 if out_f32 else 0)
    L.check(L.load().usseg_gemm_nt_batched(C.byref(d), x.data_ptr(), w.data_ptr(), y.data_ptr(), _stream()), "gemm_nt_batched")


def gemm_tn_batched(a, b, out, M, N, K, lda, ldb, nb1, nb2, as_, bs, os):
    """OUT[b1,b2][m][n] += sum_r A[b1,b2][r][m] B[b1,b2][r][n] (fp32 out, zero it first)."""
    d = GemmDesc(M, N, K, lda, ldb, N, nb1, nb2, as_[0], as_[1], bs[0], bs[1], os[0], os[1], 0)
    L.check(L.load().usseg_gemm_tn_batched(C.byref(d), a.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()), "gemm_tn_batched")


def softmax_rows_fwd(s, n, scale, p32, pbf):
    L.check(L.load().usseg_softmax_rows_fwd(s.data_ptr(), s.numel() // n, n, scale, p32.data_ptr(), pbf.data_ptr(), _stream()), "softmax_rows_fwd")


def softmax_rows_bwd(p32, dp, n, scale, ds):
    L.check(L.load().usseg_softmax_rows_bwd(p32.data_ptr(), dp.data_ptr(), p32.numel() // n, n, scale, ds.data_ptr(), _stream()), "softmax_rows_bwd")


def _dense_f32(t, n, what):
    """The attention kernels index lse / delta as dense [B*heads][N] and out32 as dense [B][N][hidden] fp32."""
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, \
        f"{what}: expected a dense fp32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)} strides {t.stride()}"


def flash_attn_fwd(qkv, nh, scale, out, lse, out32=None):
    """qkv [B,N,1,3*hidden] bf16 -> out [B,N,1,hidden] = softmax(scale q k^T) v per (image, head); lse fp32 [B*nh, N] (base 2);
    out32: optional dense fp32 copy of out (for the backward's delta)."""
    B, N, _, C3 = qkv.shape
    hs = C3 // 3
    _dense_f32(lse, B * nh * N, "lse")
    if out32 is not None:
        _dense_f32(out32, B * N * hs, "out32")
    d = L.FlashDesc(B, N, nh, hs // nh, geom(qkv)[4], geom(out)[4], scale)
    e = qkv.element_size()
    L.check(L.load().usseg_flash_attn_fwd(C.byref(d), qkv.data_ptr(), qkv.data_ptr() + hs * e, qkv.data_ptr() + 2 * hs * e, out.data_ptr(),
                                          _ptr(out32), lse.data_ptr(), _stream()), "flash_attn_fwd")
    return out


def flash_attn_bwd(qkv, nh, scale, out, d_out, lse, delta, dqkv, out32=None):
    """dqkv [B,N,1,3*hidden] bf16 (written): gradients of q, k, v slices; recomputes the probabilities from lse."""
    B, N, _, C3 = qkv.shape
    hs = C3 // 3
    assert geom(dqkv)[4] == geom(qkv)[4] and geom(d_out)[4] == geom(out)[4]
    for t, n, what in ((lse, B * nh * N, "lse"), (delta, B * nh * N, "delta"), (out32, B * N * hs, "out32")):
        if t is not None:
            _dense_f32(t, n, what)
    d = L.FlashDesc(B, N, nh, hs // nh, geom(qkv)[4], geom(out)[4], scale)
    e = qkv.element_size()
    L.check(L.load().usseg_flash_attn_bwd(C.byref(d), qkv.data_ptr(), qkv.data_ptr() + hs * e, qkv.data_ptr() + 2 * hs * e, out.data_ptr(),
                                          _ptr(out32), d_out.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), dqkv.data_ptr() + hs * e,
                                          dqkv.data_ptr() + 2 * hs * e, _stream()), "flash_attn_bwd")
    return dqkv


def transpose_batched(src, R, Cc, lds, nb1, nb2, ss, dst):
    L.check(L.load().usseg_transpose_batched(src.data_ptr(), R, Cc, lds, nb1, nb2, ss[0], ss[1], dst.data_ptr(), _stream()), "transpose_batched")


def cast_f32_to_bf16_batched(src, R, Cc, nb1, nb2, dst, ldd, ds):
    L.check(L.load().usseg_cast_f32_to_bf16_batched(src.data_ptr(), R, Cc, nb1, nb2, dst.data_ptr(), ldd, ds[0], ds[1], _stream()),
            "cast_f32_to_bf16_batched")


# ------------------------------------------------------------------------------------------------ windowed-attention encoder (Swin)
def patchify(x: torch.Tensor, patch: int) -> torch.Tensor:
    """fp32/fp64 [B,H,W,C] -> bf16 [B,H/p,W/p,roundup(p*p*C,8)]: the space-to-depth half of Conv2D(kernel = stride = p)."""
    assert x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.float64)
    B, H, W, Cc = x.shape
    Cp = roundup(patch * patch * Cc, 8)
    out = new_act(B, H // patch, W // patch, Cp, x.device)
    L.check(L.load().usseg_patchify(x.data_ptr(), 1 if x.dtype == torch.float64 else 0, B, H, W, Cc, patch, out.data_ptr(), Cp, _stream()), "patchify")
    return out


def patch_merge(full, merged, backward=False):
    """full [B,H,W,C] <-> merged [B,H/2,W/2,4C] in the reference's order x0=(0,0), x1=(1,0), x2=(0,1), x3=(1,1)."""
    B, H, W, Cc, ldf = geom(full)
    L.check(L.load().usseg_patch_merge(full.data_ptr(), B, H, W, Cc, ldf, merged.data_ptr(), geom(merged)[4], 1 if backward else 0, _stream()), "patch_merge")


def ln_wide_fwd(x, gamma, beta, eps, out):
    B, H, W, Cc, ldx = geom(x)
    L.check(L.load().usseg_ln_wide_fwd(x.data_ptr(), B * H * W, Cc, ldx, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), geom(out)[4], _stream()),
            "ln_wide_fwd")
    return out


def ln_wide_bwd(x, dy, gamma, eps, dx, dgamma, dbeta):
    B, H, W, Cc, ldx = geom(x)
    ws = reduce_ws(x.device)
    L.check(L.load().usseg_ln_wide_bwd(x.data_ptr(), dy.data_ptr(), B * H * W, Cc, ldx, geom(dy)[4], gamma.data_ptr(), eps, dx.data_ptr(), geom(dx)[4],
                                       dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ln_wide_bwd")
    return dx


def window_attn_fwd(qkv, table, heads, ws, shift, out):
    B, H, W, C3, ldq = geom(qkv)
    L.check(L.load().usseg_window_attn_fwd(qkv.data_ptr(), ldq, table.data_ptr(), B, H, W, C3 // 3, heads, ws, shift, out.data_ptr(), geom(out)[4], _stream()),
            "window_attn_fwd")
    return out


def window_attn_bwd(qkv, dout, table, heads, ws, shift, dqkv, dtable):
    B, H, W, C3, ldq = geom(qkv)
    # the kernel writes dqkv with qkv's row stride
    assert tuple(dqkv.shape) == tuple(qkv.shape) and geom(dqkv)[4] == ldq, "dqkv must have qkv's shape and row stride"
    lib = L.load()
    rows = torch.empty(int(lib.usseg_window_attn_bwd_ws_floats(B, H, W, heads, ws)), dtype=torch.float32, device=qkv.device)
    L.check(lib.usseg_window_attn_bwd(qkv.data_ptr(), ldq, dout.data_ptr(), geom(dout)[4], table.data_ptr(), B, H, W, C3 // 3, heads, ws, shift,
                                      dqkv.data_ptr(), dtable.data_ptr(), rows.data_ptr(), _stream()), "window_attn_bwd")
    return dqkv


def token_mean_fwd(x):
    B, H, W, Cc, ld = geom(x)
    out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    L.check(L.load().usseg_token_mean_fwd(x.data_ptr(), B, H * W, Cc, ld, out.data_ptr(), _stream()), "token_mean_fwd")
    return out


def token_mean_bwd(dy, like):
    B, H, W, Cc, _ = geom(like)
    dx = torch.empty(like.shape, dtype=like.dtype, device=like.device)      # dense: the kernel writes it with dx's own row stride
    L.check(L.load().usseg_token_mean_bwd(dy.data_ptr(), B, H * W, Cc, geom(dx)[4], dx.data_ptr(), _stream()), "token_mean_bwd")
    return dx


# ------------------------------------------------------------------------------------------------ offline preprocessing (prep.hip)
PREP_H, PREP_W = L.PREP_H, L.PREP_W


def _prep_check(t, name, dtype, ndim):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == ndim and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dtype} cuda tensor of {ndim} dims")


def prep_cycle_stats(frames):
    """frames fp64 [C,10,H0,W0] -> stats fp64 [C*10,2]: each plane's mean and safe_max (DataFilePlayGround.py:368-376)."""
    _prep_check(frames, "frames", torch.float64, 4)
    Cc, K, H0, W0 = frames.shape
    if K != 10:
        raise ValueError(f"frames must hold 10 planes per cycle, has {K}")
    col = torch.empty((Cc * 10, 3, W0), dtype=torch.float64, device=frames.device)
    stats = torch.empty((Cc * 10, 2), dtype=torch.float64, device=frames.device)
    L.check(L.load().usseg_prep_cycle_stats(frames.data_ptr(), Cc, H0, W0, col.data_ptr(), stats.data_ptr(), _stream()), "prep_cycle_stats")
    return stats


def prep_label(brain, objective, blood=None, normal=None):
    """The label fp32 [256,80] and the gate uint8 [256,80] (1 where the resized brain mask is 0) of one file (DataFilePlayGround.py:330-343).
    brain fp64 [Hb,Wb]; objective 1 also takes blood and normal fp64 [Hm,Wm]."""
    _prep_check(brain, "brain", torch.float64, 2)
    Hm = Wm = 0
    ws = None
    if objective == 1:
        _prep_check(blood, "blood", torch.float64, 2)
        _prep_check(normal, "normal", torch.float64, 2)
        if blood.shape != normal.shape:
            raise ValueError(f"blood {tuple(blood.shape)} and normal {tuple(normal.shape)} masks differ in shape")
        Hm, Wm = blood.shape
        ws = torch.empty((2, Hm * Wm), dtype=torch.float32, device=brain.device)
    label = torch.empty((PREP_H, PREP_W), dtype=torch.float32, device=brain.device)
    gate = torch.empty((PREP_H, PREP_W), dtype=torch.uint8, device=brain.device)
    L.check(L.load().usseg_prep_label(brain.data_ptr(), brain.shape[0], brain.shape[1], _ptr(blood if objective == 1 else None),
                                      _ptr(normal if objective == 1 else None), Hm, Wm, objective, _ptr(ws), label.data_ptr(), gate.data_ptr(),
                                      _stream()), "prep_label")
    return label, gate


def prep_label_thick(brain, blood, order):
    """The label fp32 [256,80] and the gate uint8 [256,80] from bloodMaskThick, no blur (PizzaPlayGround.py:92-97, order 0;
    DataPreprocessing.py:134-146, order 1).  brain fp64 [Hb,Wb], blood fp64 [Hm,Wm]; the rules are in include/usseg.h."""
    _prep_check(brain, "brain", torch.float64, 2)
    _prep_check(blood, "blood", torch.float64, 2)
    if order not in (0, 1):
        raise ValueError(f"order must be 0 (PizzaPlayGround) or 1 (DataPreprocessing), got {order!r}")
    if brain.device != blood.device:
        raise ValueError("prep_label_thick: brain and blood are on different devices")
    label = torch.empty((PREP_H, PREP_W), dtype=torch.float32, device=brain.device)
    gate = torch.empty((PREP_H, PREP_W), dtype=torch.uint8, device=brain.device)
    L.check(L.load().usseg_prep_label_thick(brain.data_ptr(), brain.shape[0], brain.shape[1], blood.data_ptr(), blood.shape[0], blood.shape[1],
                                            int(order), label.data_ptr(), gate.data_ptr(), _stream()), "prep_label_thick")
    return label, gate


def select_ranks_f64(x, ranks, active=None):
    """x fp64 [N,n] -> fp64 [N,len(ranks)]: the value of each rank (0 = the smallest, at most 4 ranks) of every row, exact (a radix select
    on the device; a zero comes back as +0.0).  active (int32 [N], optional): rows whose entry is 0 are skipped and come back as NaN."""
    _prep_check(x, "x", torch.float64, 2)
    ranks = [int(r) for r in ranks]
    if active is not None:
        _prep_check(active, "active", torch.int32, 1)
        if active.shape[0] != x.shape[0] or active.device != x.device:
            raise ValueError("select_ranks_f64: active must hold one entry per row of x, on its device")
    out = torch.full((x.shape[0], len(ranks)), float("nan"), dtype=torch.float64, device=x.device)
    L.check(L.load().usseg_select_ranks_f64(x.data_ptr(), x.shape[0], x.shape[1], (C.c_int32 * max(len(ranks), 1))(*ranks), len(ranks),
                                            _ptr(active), out.data_ptr(), _stream()), "select_ranks_f64")
    return out


def prep_aug(images, table, rot_list, n_rot, k_lo, g_lo, k_hi, g_hi, zH, zW, noise=None, noise_out=None):
    """DataFilePlayGround.dataAug of a batch in seven launches (csrc/prep_aug.hip): images fp64 [N,H,W,Cc] -> a new fp64 [N,H,W,Cc].
    table: uint8 tensor holding N UssegPrepAugSample; rot_list int32 [>= max(n_rot, 1)]; (k, g) the floor and fraction of the 2nd and 98th
    percentile's position among H*W*Cc values; zH, zW = (sqrt(3)-2)^(H-1), ^(W-1); noise / noise_out fp64 [N,H,W,Cc-1] or None."""
    _prep_check(images, "images", torch.float64, 4)
    _prep_check(table, "table", torch.uint8, 1)
    _prep_check(rot_list, "rot_list", torch.int32, 1)
    N, H, W, Cc = images.shape
    if table.numel() != N * C.sizeof(L.PrepAugSample) or rot_list.numel() < max(n_rot, 1):
        raise ValueError("prep_aug: table or rot_list does not match the batch")
    for t, name in ((noise, "noise"), (noise_out, "noise_out")):
        if t is not None:
            _prep_check(t, name, torch.float64, 4)
            if tuple(t.shape) != (N, H, W, Cc - 1):
                raise ValueError(f"prep_aug: {name} must be [N, H, W, Cc-1] = {(N, H, W, Cc - 1)}, is {tuple(t.shape)}")
    lib = L.load()
    need = lib.usseg_prep_aug_ws_doubles(N, H, W, Cc, n_rot)
    if need < 0:
        raise ValueError(f"prep_aug: bad geometry {tuple(images.shape)}, n_rot {n_rot}")
    ws = torch.empty(need, dtype=torch.float64, device=images.device)
    out = torch.empty_like(images)
    d = L.PrepAugDesc(N, H, W, Cc, n_rot, k_lo, k_hi, g_lo, g_hi, zH, zW)
    L.check(lib.usseg_prep_aug(C.byref(d), table.data_ptr(), rot_list.data_ptr(), images.data_ptr(), _ptr(noise), ws.data_ptr(), need,
                               out.data_ptr(), _ptr(noise_out), _stream()), "prep_aug")
    return out


def prep_assemble(frames, stats, bmode, label, gate, objective):
    """The images of every cycle of one file: fp64 [C,1,256,80,12] (DataFilePlayGround.py:353-393).  frames fp64 [C,10,H0,W0], stats from
    prep_cycle_stats, bmode fp64 [C,Hq,Wq,F] (bModeNorm with the cycle axis first), label / gate from prep_label."""
    _prep_check(frames, "frames", torch.float64, 4)
    _prep_check(stats, "stats", torch.float64, 2)
    _prep_check(bmode, "bmode", torch.float64, 4)
    _prep_check(label, "label", torch.float32, 2)
    _prep_check(gate, "gate", torch.uint8, 2)
    Cc, _, H0, W0 = frames.shape
    if tuple(stats.shape) != (Cc * 10, 2) or bmode.shape[0] != Cc or tuple(label.shape) != (PREP_H, PREP_W) or label.shape != gate.shape:
        raise ValueError("prep_assemble: stats, bmode, label and gate do not match the frames")
    out = torch.empty((Cc, 1, PREP_H, PREP_W, 12), dtype=torch.float64, device=frames.device)
    L.check(L.load().usseg_prep_assemble(frames.data_ptr(), stats.data_ptr(), Cc, H0, W0, bmode.data_ptr(), bmode.shape[1], bmode.shape[2],
                                         bmode.shape[3], label.data_ptr(), gate.data_ptr(), objective, out.data_ptr(), _stream()), "prep_assemble")
    return out


# ------------------------------------------------------------------------------------------------ the evaluator's cone figures (cone.hip)
_INT32_MAX = 2**31 - 1


def cone_index(X, Y, xmin, ymin, px_per_unit, Hp, Wp):
    """Which quad of the vertex grid X, Y (fp64 [H,W]) each pixel of a [Hp,Wp] panel shows: -> int32 [Hp,Wp], -1 for background.
    Pixel (r, c) samples (xmin + (c+0.5)/px_per_unit, ymin + (r+0.5)/px_per_unit) (include/usseg.h, usseg_cone_index)."""
    _prep_check(X, "X", torch.float64, 2)
    _prep_check(Y, "Y", torch.float64, 2)
    if X.shape != Y.shape or X.device != Y.device or min(X.shape) < 2:
        raise ValueError(f"X {tuple(X.shape)} and Y {tuple(Y.shape)} must be one [H,W] grid (H, W >= 2) on one device")
    if X.numel() * 8 > _INT32_MAX or not (1 <= Hp and 1 <= Wp and Hp * Wp * 4 <= _INT32_MAX):
        raise ValueError(f"grid {tuple(X.shape)} / panel {Hp}x{Wp}: empty, or byte offsets overflow int32")
    if not (math.isfinite(px_per_unit) and px_per_unit > 0 and math.isfinite(xmin) and math.isfinite(ymin)):
        raise ValueError(f"bad origin ({xmin}, {ymin}) or px_per_unit {px_per_unit}")
    index = torch.empty((Hp, Wp), dtype=torch.int32, device=X.device)
    L.check(L.load().usseg_cone_index(X.data_ptr(), Y.data_ptr(), X.shape[0], X.shape[1], float(xmin), float(ymin), float(px_per_unit), Hp, Wp,
                                      index.data_ptr(), _stream()), "cone_index")
    return index


def cone_range(bmode):
    """bmode fp64 [B,H,W] -> (range fp64 [B,2]: np.histogram(bmode[b], bins=25)[1][[2, -2]], nonfinite int32 [B]: nonzero where
    np.histogram would raise - bit 0 a NaN or an infinity, bit 1 edges that do not strictly increase)."""
    _prep_check(bmode, "bmode", torch.float64, 3)
    B = bmode.shape[0]
    if not (1 <= B <= 65535) or bmode[0].numel() < 1:
        raise ValueError(f"bmode {tuple(bmode.shape)}: 1..65535 non-empty images")
    rng = torch.empty((B, 2), dtype=torch.float64, device=bmode.device)
    bad = torch.empty((B,), dtype=torch.int32, device=bmode.device)
    L.check(L.load().usseg_cone_range(bmode.data_ptr(), B, bmode[0].numel(), rng.data_ptr(), bad.data_ptr(), _stream()), "cone_range")
    return rng, bad


def cone_render(index, prob_map, label, bleed_prob, bmode, ranges, bmode_range, luts, gap):
    """The four panels of every image: -> uint8 [B, 2*Hp+gap, 2*Wp+gap, 3] (usseg_cone_render).  index int32 [Hp,Wp] from cone_index;
    prob_map, bleed_prob fp32 and label, bmode fp64 [B,H,W]; ranges: three (vmin, vmax) pairs of panels 0..2 (host numbers);
    bmode_range fp64 [B,2] from cone_range; luts uint8 [2,256,3] (panels 0-2, panel 3)."""
    _prep_check(index, "index", torch.int32, 2)
    for name, t, dt in (("prob_map", prob_map, torch.float32), ("label", label, torch.float64), ("bleed_prob", bleed_prob, torch.float32),
                        ("bmode", bmode, torch.float64)):
        _prep_check(t, name, dt, 3)
        if t.shape != prob_map.shape:
            raise ValueError(f"{name} {tuple(t.shape)} and prob_map {tuple(prob_map.shape)} differ in shape")
    _prep_check(bmode_range, "bmode_range", torch.float64, 2)
    _prep_check(luts, "luts", torch.uint8, 3)
    B, H, W = prob_map.shape
    Hp, Wp = index.shape
    if tuple(bmode_range.shape) != (B, 2) or tuple(luts.shape) != (2, 256, 3):
        raise ValueError(f"bmode_range {tuple(bmode_range.shape)} must be [{B},2] and luts {tuple(luts.shape)} [2,256,3]")
    if len({t.device for t in (index, prob_map, label, bleed_prob, bmode, bmode_range, luts)}) != 1:
        raise ValueError("cone_render: the tensors are on more than one device")
    r = [float(v) for pair in ranges for v in pair]
    if len(r) != 6:
        raise ValueError(f"ranges must be three (vmin, vmax) pairs, got {ranges!r}")
    gap = int(gap)
    OH, OW = 2 * Hp + gap, 2 * Wp + gap
    if gap < 0 or H < 2 or W < 2 or OH * OW * 3 > _INT32_MAX or H * W * 8 > _INT32_MAX:
        raise ValueError(f"cone_render: bad gap {gap} or planes [{B},{H},{W}], or a {OH}x{OW} figure overflows int32 byte offsets")
    out = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device=index.device)
    L.check(L.load().usseg_cone_render(index.data_ptr(), Hp, Wp, gap, prob_map.data_ptr(), label.data_ptr(), bleed_prob.data_ptr(),
                                       bmode.data_ptr(), B, H, W, (C.c_double * 6)(*r), bmode_range.data_ptr(), luts.data_ptr(), out.data_ptr(),
                                       _stream()), "cone_render")
    return out
