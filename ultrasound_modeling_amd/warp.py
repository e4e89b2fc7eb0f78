"""Random elastic deformation with a small rotation, scale and translation for TRAINING batches, on the device (not in the reference).

The reference's online augmentation (``DataAugs.dataAug``) reduces, clips, shifts by whole pixels and adds noise; nothing in it deforms the
anatomy.  This is the standard remedy for a small segmentation set (Simard et al. 2003; the U-Net paper; nnU-Net): per sample a uniform random
field is smoothed with a Gaussian of ``sigma`` pixels, scaled to a target RMS displacement and added to an affine map of the output grid; the
image is sampled there bilinearly and the label by nearest neighbour (labels are continuous values that ``label2vec`` thresholds, so nothing
may interpolate them).  ``usseg_elastic_warp`` (csrc/warp.hip, two launches per batch; semantics in include/usseg.h and DESIGN.md section 4h-2)
does the work; the DRAWS stay on the host, from a ``random.Random`` of their own, so the reference's sequence of boxes and shifts
(``DataAugs.draw``) is the same with and without warping.  ``Dataset_2.Dataset(warp=...)`` warps a training batch FIRST and hands the warped
``x`` and ``y`` to ``dataAug_batch``; validation batches are never warped.

``cfg`` (``warp_config`` / ``parse_warp``):
  sigma      smoothing in pixels, 0 < sigma <= 16 (the kernel's radius is int(4*sigma + 0.5) <= 64)
  magnitude  (rows, cols): the target RMS displacement in pixels.  alpha = magnitude * sigma * sqrt(12*pi): a uniform [-1, 1) field has
             variance 1/3 and the 2-D Gaussian keeps 1 / (4*pi*sigma^2) of it.  The smoothing pads with zeros, so the displacement is SMALLER
             than this within about 2*sigma of the borders.
  p          probability that a sample is warped (the others are copied bit for bit)
  rotate     degrees; theta is drawn uniform on +-rotate
  scale      the log of the scale factor is drawn uniform on +-scale
  shift      (rows, cols): the translation is drawn uniform on +- these pixel amounts
The defaults (sigma 8, magnitude 2:1, p 0.5, rotate 5, scale 0.05, no shift) are ordinary choices from the literature.  NOBODY HAS MEASURED
their effect on this data.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import numpy as np

DEFAULTS = {"sigma": 8.0, "magnitude": (2.0, 1.0), "p": 0.5, "rotate": 5.0, "scale": 0.05, "shift": (0.0, 0.0)}
MAX_SIGMA = 16.0


def _pair(name, v):
    if isinstance(v, (int, float)):
        v = (v, v)
    try:
        a, b = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError(f"warp: {name} takes one number or two (rows, cols), got {v!r}")
    if not (math.isfinite(a) and math.isfinite(b) and a >= 0 and b >= 0):
        raise ValueError(f"warp: {name} must be finite and >= 0, got {v!r}")
    return (a, b)


def warp_config(cfg=None) -> dict:
    """A checked copy of ``cfg`` (a dict, a ``parse_warp`` string or None) with the defaults filled in; ``ValueError`` for an unknown key or a
    value out of range."""
    if isinstance(cfg, str):
        return parse_warp(cfg)
    cfg = {} if cfg is None else cfg
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f"warp: a dict with keys from {sorted(DEFAULTS)}, got {cfg!r}")
    out = dict(DEFAULTS, **cfg)
    for k in ("sigma", "p", "rotate", "scale"):
        try:
            out[k] = float(out[k])
        except (TypeError, ValueError):
            raise ValueError(f"warp: {k} must be a number, got {out[k]!r}")
    if not 0 < out["sigma"] <= MAX_SIGMA:
        raise ValueError(f"warp: 0 < sigma <= {MAX_SIGMA:g}, got {out['sigma']!r}")
    if not 0 <= out["p"] <= 1:
        raise ValueError(f"warp: 0 <= p <= 1, got {out['p']!r}")
    if not 0 <= out["rotate"] <= 180:
        raise ValueError(f"warp: 0 <= rotate <= 180 degrees, got {out['rotate']!r}")
    if not 0 <= out["scale"] <= 1:
        raise ValueError(f"warp: 0 <= scale <= 1 (the log of the factor), got {out['scale']!r}")
    out["magnitude"] = _pair("magnitude", out["magnitude"])
    out["shift"] = _pair("shift", out["shift"])
    return out


def parse_warp(spec: str) -> dict:
    """``"sigma=8,magnitude=2:1,p=0.5,rotate=5,scale=0.05,shift=0:0"`` (any subset, any order; the empty string is the defaults) -> ``cfg``."""
    if not isinstance(spec, str):
        raise ValueError(f"warp: a string of key=value pairs, got {spec!r}")
    cfg = {}
    for item in filter(None, (t.strip() for t in spec.split(","))):
        key, eq, val = item.partition("=")
        key = key.strip()
        if not eq or key not in DEFAULTS or key in cfg:
            raise ValueError(f"warp: bad item {item!r} in {spec!r} (keys: {', '.join(DEFAULTS)}; each at most once)")
        try:
            nums = [float(t) for t in val.split(":")]
        except ValueError:
            raise ValueError(f"warp: bad number in {item!r}")
        if key in ("magnitude", "shift"):
            if len(nums) not in (1, 2):
                raise ValueError(f"warp: {key} takes ROWS:COLS or one number, got {item!r}")
            cfg[key] = tuple(nums) if len(nums) == 2 else nums[0]
        else:
            if len(nums) != 1:
                raise ValueError(f"warp: {key} takes one number, got {item!r}")
            cfg[key] = nums[0]
    return warp_config(cfg)


def format_warp(cfg: dict) -> str:
    """The ``parse_warp`` string of a ``cfg``: ``parse_warp(format_warp(cfg)) == cfg``."""
    cfg = warp_config(cfg)
    return ",".join(f"{k}={cfg[k][0]!r}:{cfg[k][1]!r}" if k in ("magnitude", "shift") else f"{k}={cfg[k]!r}" for k in DEFAULTS)


def gaussian_radius(sigma: float) -> int:
    return int(4.0 * float(sigma) + 0.5)


def gaussian_weights(sigma: float) -> np.ndarray:
    """fp64 [radius + 1], w[0] the centre tap: exp(-0.5 k^2 / sigma^2) over k = -radius..radius normalised to sum 1, radius = int(4*sigma + 0.5)
    (the table of ``scipy.ndimage.gaussian_filter(sigma, truncate=4.0)``)."""
    r = gaussian_radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * k * k)
    w /= w.sum()
    return np.ascontiguousarray(w[r:])


def alpha_of(cfg: dict):
    """(rows, cols) multipliers of the smoothed unit field that give the target RMS displacement (module docstring)."""
    g = cfg["sigma"] * math.sqrt(12.0 * math.pi)
    return (cfg["magnitude"][0] * g, cfg["magnitude"][1] * g)


def affine_of(theta_deg: float, log_scale: float, shift, H: int, W: int):
    """[A00, A01, A10, A11, o0, o1] of src = c + A (p - c) + shift with c = ((H-1)/2, (W-1)/2) and A = exp(log_scale) * rotation(theta): the
    map from an OUTPUT pixel p = (i, j) to its source coordinate, the centre folded into o."""
    t, s = math.radians(theta_deg), math.exp(log_scale)
    a00, a01, a10, a11 = s * math.cos(t), -s * math.sin(t), s * math.sin(t), s * math.cos(t)
    c0, c1 = (H - 1) / 2.0, (W - 1) / 2.0
    return [a00, a01, a10, a11, c0 - (a00 * c0 + a01 * c1) + shift[0], c1 - (a10 * c0 + a11 * c1) + shift[1]]


def draw_warp(rng, cfg: dict, H: int, W: int) -> dict:
    """One sample's draws from ``rng`` (a ``random.Random`` of the warp's own), always six in the same order - active, seed, theta, log scale, two
    shifts - whether or not the sample turns out active.  -> ``active``, ``seed``, ``alpha`` (rows, cols), ``aff`` (``affine_of``) and the drawn
    ``theta`` (degrees), ``log_scale`` and ``shift``."""
    active = rng.random() < cfg["p"]
    seed = rng.getrandbits(63)
    theta = rng.uniform(-cfg["rotate"], cfg["rotate"])
    log_scale = rng.uniform(-cfg["scale"], cfg["scale"])
    shift = (rng.uniform(-cfg["shift"][0], cfg["shift"][0]), rng.uniform(-cfg["shift"][1], cfg["shift"][1]))
    return {"active": active, "seed": seed, "alpha": alpha_of(cfg), "aff": affine_of(theta, log_scale, shift, H, W), "theta": theta,
            "log_scale": log_scale, "shift": shift}


def sample_table(params: List[dict], device):
    """The device table of ``UssegWarpSample`` that ``usseg_elastic_warp`` reads on every launch -> uint8 tensor [len(params) * 80]."""
    import torch
    from . import _lib as L
    arr = (L.WarpSample * len(params))()
    for i, p in enumerate(params):
        s = arr[i]
        s.active, s.seed = int(bool(p["active"])), int(p["seed"]) & ((1 << 64) - 1)
        s.alpha[0], s.alpha[1] = (float(v) for v in p["alpha"])
        for q in range(6):
            s.aff[q] = float(p["aff"][q])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


_WEIGHTS = {}


def device_weights(sigma: float, device):
    """``gaussian_weights(sigma)`` on ``device`` (kept: a table per sigma and device)."""
    import torch
    key = (float(sigma), str(device))
    if key not in _WEIGHTS:
        _WEIGHTS[key] = torch.from_numpy(gaussian_weights(sigma)).to(device)
    return _WEIGHTS[key]


def elastic_warp(x, y, table, weights, field=None, want_debug: bool = False, out=None):
    """``usseg_elastic_warp`` on the current stream: x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32 (contiguous, on the device), ``table`` of
    ``sample_table``, ``weights`` fp64 [radius + 1] on the device, ``field`` fp64 [B,2,H,W] or None -> (x_out, y_out[, disp, field_used]).
    ``out``: (x_out, y_out) to write into (a captured graph's static buffers).  Nothing synchronises; the workspace comes from torch's
    caching allocator."""
    import torch
    from . import _lib as L
    if not (x.is_cuda and y.is_cuda and table.is_cuda and weights.is_cuda):
        raise RuntimeError("elastic_warp runs on the GPU only: there is no CPU fallback")
    if x.dim() != 4 or y.dim() != 3 or x.dtype not in (torch.float32, torch.float64) or y.dtype != torch.float32 or tuple(y.shape) != tuple(x.shape[:3]):
        raise ValueError(f"elastic_warp: x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32, got {tuple(x.shape)} {x.dtype} and {tuple(y.shape)} {y.dtype}")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("elastic_warp: x and y must be contiguous")
    B, H, W, Cc = x.shape
    radius = int(weights.numel()) - 1
    if weights.dtype != torch.float64 or not 0 <= radius <= L.WARP_MAX_RADIUS:
        raise ValueError(f"elastic_warp: weights fp64 [radius + 1] with 0 <= radius <= {L.WARP_MAX_RADIUS}, got {tuple(weights.shape)} {weights.dtype}")
    if table.numel() * table.element_size() != B * C.sizeof(L.WarpSample):
        raise ValueError(f"elastic_warp: a table of {B} samples, got {table.numel() * table.element_size()} bytes")
    if field is not None and (field.dtype != torch.float64 or tuple(field.shape) != (B, 2, H, W) or not field.is_cuda or not field.is_contiguous()):
        raise ValueError(f"elastic_warp: field fp64 [B,2,H,W] contiguous on the device, got {tuple(field.shape)} {field.dtype}")
    lib = L.load()
    xo, yo = (torch.empty_like(x), torch.empty_like(y)) if out is None else out
    if xo.shape != x.shape or xo.dtype != x.dtype or yo.shape != y.shape or yo.dtype != y.dtype or not (xo.is_contiguous() and yo.is_contiguous()):
        raise ValueError("elastic_warp: out must match x and y in shape and dtype and be contiguous")
    disp = torch.empty((B, 2, H, W), dtype=torch.float64, device=x.device) if want_debug else None
    used = torch.empty((B, 2, H, W), dtype=torch.float64, device=x.device) if want_debug else None
    ws_bytes = int(lib.usseg_warp_ws_bytes(B, H, W))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
    d = L.WarpDesc(B, H, W, Cc, 1 if x.dtype == torch.float64 else 0, radius)
    L.check(lib.usseg_elastic_warp(C.byref(d), table.data_ptr(), weights.data_ptr(), None if field is None else field.data_ptr(), x.data_ptr(),
                                   y.data_ptr(), ws.data_ptr(), ws_bytes, xo.data_ptr(), yo.data_ptr(), None if disp is None else disp.data_ptr(),
                                   None if used is None else used.data_ptr(), torch.cuda.current_stream().cuda_stream), "elastic_warp")
    return (xo, yo, disp, used) if want_debug else (xo, yo)


def warp_batch(x, y, params: List[dict], cfg: dict, field=None, want_debug: bool = False):
    """x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32 ON THE DEVICE, ``params`` one ``draw_warp`` dict per sample -> (x_warped, y_warped[, disp,
    field]) of the same shapes and dtypes; ``disp`` / ``field`` fp64 [B,2,H,W]: the displacement in pixels and the random field that was used."""
    if len(params) != x.shape[0]:
        raise ValueError(f"warp_batch: {len(params)} parameter sets for {x.shape[0]} samples")
    return elastic_warp(x.contiguous(), y.contiguous(), sample_table(params, x.device), device_weights(cfg["sigma"], x.device), field=field,
                        want_debug=want_debug)
