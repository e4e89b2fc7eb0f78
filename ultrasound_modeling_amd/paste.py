"""Lesion copy-paste augmentation for TRAINING batches, on the device (not in the reference).

Bleed pixels are rare, and every loss and sampler here reweights or repeats the ones that exist.  Copy-paste (Ghiasi et al., "Simple Copy-Paste",
CVPR 2021; TumorCP and CarveMix for medical lesions) makes NEW positive examples: a labelled lesion of one training record - a connected component
of ``label >= 1.05``, ``label2vec``'s bleed threshold - is put, pixels and label, into another record's brain (``label > 0.95``).  The whole
training set is resident in HBM, so the bank of lesions is the training set itself plus one int32 label image (``LesionBank``), and
``usseg_lesion_paste`` (csrc/paste.hip, two launches per batch; semantics in include/usseg_paste.h and DESIGN.md section 4h-3) gathers straight
from it.  The DRAWS stay on the host, from a ``random.Random`` of their own, so the sequences of ``DataAugs.draw`` and of the warp are the same
with and without pasting.  ``Dataset_2.Dataset(paste=...)`` pastes into a training batch FIRST, then warps (``warp=``), then hands ``x`` and
``y`` to ``dataAug_batch``; validation batches are never pasted.

``cfg`` (``paste_config`` / ``parse_paste``):
  p            probability that a sample receives lesions (the others are copied bit for bit)
  max_lesions  an active sample draws 1..max_lesions lesions, 1 <= max_lesions <= 4 (USSEG_PASTE_MAX_ITEMS)
  min_area     lesions of fewer pixels are not in the bank
  min_landed   a drawn lesion is placed only if at least max(1, ceil(min_landed * area)) of its pixels land on recipient brain
  flip         mirror a drawn lesion left-right with probability 0.5
  shift        None: the lesion goes anywhere its bounding box fits; (rows, cols): it moves by at most that many pixels from where it lay
  protect      never paste over the recipient's own bleed
  connectivity 4 or 8: what makes one lesion (``ops.label_components``)
The defaults (p 0.5, max_lesions 2, min_area 4, min_landed 0.5, flip, anywhere, protect, 8) are ordinary choices from the literature.  NOBODY HAS
MEASURED their effect on this data.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List

import numpy as np

DEFAULTS = {"p": 0.5, "max_lesions": 2, "min_area": 4, "min_landed": 0.5, "flip": True, "shift": None, "protect": True, "connectivity": 8}
MAX_ITEMS = 4           # USSEG_PASTE_MAX_ITEMS (checked against the header by LesionBank and sample_table, which load the binding)
_BOOLS = {"1": True, "true": True, "yes": True, "on": True, "0": False, "false": False, "no": False, "off": False}


def _whole(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (math.inf, -math.inf) or int(v) != v:
        raise ValueError(f"paste: {name} must be a whole number, got {v!r}")
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"paste: {name} must be >= {lo}" + (f" and <= {hi}" if hi is not None else "") + f", got {v!r}")
    return v


def _flag(name, v):
    if isinstance(v, bool):
        return v
    if isinstance(v, (int, float)) and v in (0, 1):
        return bool(v)
    raise ValueError(f"paste: {name} must be True or False, got {v!r}")


def paste_config(cfg=None) -> dict:
    """A checked copy of ``cfg`` (a dict, a ``parse_paste`` string or None) with the defaults filled in; ``ValueError`` for an unknown key or a
    value out of range."""
    if isinstance(cfg, str):
        return parse_paste(cfg)
    cfg = {} if cfg is None else cfg
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f"paste: a dict with keys from {sorted(DEFAULTS)}, got {cfg!r}")
    out = dict(DEFAULTS, **cfg)
    for k in ("p", "min_landed"):
        if isinstance(out[k], bool) or not isinstance(out[k], (int, float)):
            raise ValueError(f"paste: {k} must be a number, got {out[k]!r}")
        out[k] = float(out[k])
        if not 0 <= out[k] <= 1:
            raise ValueError(f"paste: 0 <= {k} <= 1, got {out[k]!r}")
    out["max_lesions"] = _whole("max_lesions", out["max_lesions"], 1, MAX_ITEMS)
    out["min_area"] = _whole("min_area", out["min_area"], 1)
    out["flip"], out["protect"] = _flag("flip", out["flip"]), _flag("protect", out["protect"])
    if out["connectivity"] not in (4, 8) or isinstance(out["connectivity"], bool):
        raise ValueError(f"paste: connectivity must be 4 or 8, got {out['connectivity']!r}")
    out["connectivity"] = int(out["connectivity"])
    if out["shift"] is not None:
        sh = out["shift"]
        if isinstance(sh, (int, float)) and not isinstance(sh, bool):
            sh = (sh, sh)
        try:
            a, b = sh
        except (TypeError, ValueError):
            raise ValueError(f"paste: shift takes None, one whole number or two (rows, cols), got {out['shift']!r}")
        out["shift"] = (_whole("shift", a, 0), _whole("shift", b, 0))
    return out


def parse_paste(spec: str) -> dict:
    """``"p=0.5,max_lesions=2,min_area=4,min_landed=0.5,flip=1,shift=none,protect=1,connectivity=8"`` (any subset, any order; the empty string
    is the defaults; ``shift=ROWS:COLS`` or ``shift=none``) -> ``cfg``."""
    if not isinstance(spec, str):
        raise ValueError(f"paste: a string of key=value pairs, got {spec!r}")
    cfg = {}
    for item in filter(None, (t.strip() for t in spec.split(","))):
        key, eq, val = item.partition("=")
        key, val = key.strip(), val.strip().lower()
        if not eq or key not in DEFAULTS or key in cfg:
            raise ValueError(f"paste: bad item {item!r} in {spec!r} (keys: {', '.join(DEFAULTS)}; each at most once)")
        if key in ("flip", "protect"):
            if val not in _BOOLS:
                raise ValueError(f"paste: {key} takes 1 or 0, got {item!r}")
            cfg[key] = _BOOLS[val]
            continue
        if key == "shift" and val in ("none", "any"):
            cfg[key] = None
            continue
        try:
            nums = [float(t) for t in val.split(":")]
        except ValueError:
            raise ValueError(f"paste: bad number in {item!r}")
        if key == "shift":
            if len(nums) not in (1, 2):
                raise ValueError(f"paste: shift takes ROWS:COLS, one number or none, got {item!r}")
            cfg[key] = tuple(nums) if len(nums) == 2 else nums[0]
        else:
            if len(nums) != 1:
                raise ValueError(f"paste: {key} takes one number, got {item!r}")
            cfg[key] = nums[0]
    return paste_config(cfg)


def format_paste(cfg: dict) -> str:
    """The ``parse_paste`` string of a ``cfg``: ``parse_paste(format_paste(cfg)) == cfg``."""
    cfg = paste_config(cfg)

    def one(k):
        v = cfg[k]
        if k == "shift":
            return "shift=none" if v is None else f"shift={v[0]}:{v[1]}"
        return f"{k}={int(v)}" if isinstance(v, bool) else f"{k}={v!r}"
    return ",".join(one(k) for k in DEFAULTS)


# ------------------------------------------------------------------------------------------------ the bank
LESION_FIELDS = ("record", "comp", "area", "r0", "c0", "r1", "c1")
_CHUNK_PIXELS = 1 << 22         # pixels labelled per call: the labelling workspace (12 bytes a pixel) stays at 48 MB whatever N is


class LesionBank(object):
    """The lesions of a training set: ``labels`` int32 [N,H,W] ON THE DEVICE (0 outside; 1..K_n the connected components of
    ``y_tr >= 1.05`` of record n in ``scipy.ndimage.label``'s numbering) and ``table``, a host int64 [L,7] array of ``LESION_FIELDS`` - the
    lesions of at least ``min_area`` pixels, record-major, then by component id; the box is inclusive.  Built once, with the device's own
    labelling (``ops.label_components`` / ``ops.component_stats``: no new kernel), in chunks of records so that the workspace does not grow with
    N; the statistics are read back once.  ``ValueError`` for a training set without a lesion.  ``labels=`` / ``table=``: a bank made elsewhere."""

    def __init__(self, y_tr=None, connectivity=8, min_area=4, *, labels=None, table=None):
        if table is None:
            labels, table = self._build(y_tr, int(connectivity), int(min_area))
        self.labels = labels
        self.table = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, len(LESION_FIELDS)))
        self.N, self.H, self.W = (int(v) for v in labels.shape)
        if len(self.table) == 0:
            raise ValueError(f"paste: the training set holds no lesion (a connected component of label >= 1.05) of at least {int(min_area)} pixels")

    def __len__(self):
        return len(self.table)

    @staticmethod
    def _build(y_tr, connectivity, min_area):
        import torch
        from . import ops
        if not (isinstance(y_tr, torch.Tensor) and y_tr.is_cuda):
            raise RuntimeError("LesionBank labels the training set on the GPU only: there is no CPU fallback")
        if y_tr.dim() != 3 or y_tr.dtype != torch.float32 or not y_tr.is_contiguous():
            raise ValueError(f"paste: y_tr fp32 [N,H,W] contiguous, got {tuple(y_tr.shape)} {y_tr.dtype}")
        N, H, W = y_tr.shape
        step = max(1, min(_CHUNK_PIXELS // (H * W), 65535))
        labels = torch.empty((N, H, W), dtype=torch.int32, device=y_tr.device)
        count = torch.empty((N,), dtype=torch.int32, device=y_tr.device)
        ws = torch.empty(max(ops.components_ws_bytes(min(step, N), H, W), 16), dtype=torch.uint8, device=y_tr.device)
        for s in range(0, N, step):
            mask = (y_tr[s:s + step] >= 1.05).to(torch.uint8)
            ops.label_components(mask, connectivity, labels=labels[s:s + step], count=count[s:s + step], ws=ws)
        cap = int(count.max()) if N else 0
        if cap == 0:
            return labels, np.zeros((0, len(LESION_FIELDS)), np.int64)
        stats = torch.cat([ops.component_stats(labels[s:s + step], cap) for s in range(0, N, step)]).cpu().numpy()      # the one read-back
        rec, k = np.nonzero(stats[:, :, 0] >= max(min_area, 1))             # record-major, then component id
        return labels, np.concatenate([rec[:, None], k[:, None] + 1, stats[rec, k, :5]], axis=1)


# ------------------------------------------------------------------------------------------------ the draws
def _span(lo, hi, s):
    """[lo, hi] (which holds 0) intersected with [-s, s]."""
    return (lo, hi) if s is None else (max(lo, -s), min(hi, s))


def draw_paste(rng, cfg: dict, bank, H: int, W: int) -> dict:
    """One sample's draws from ``rng`` (a ``random.Random`` of the paste's own), always ``2 + 4 * max_lesions`` in the same order - active, the
    item count, then per slot a lesion, the flip, the row shift and the column shift (after the flip) - whether or not the sample turns out
    active.  -> ``active``, ``n`` (the items that count) and ``items``, ``max_lesions`` dicts of ``record, comp, dr, dc, flip, need`` with the
    donor ``box`` (r0, c0, r1, c1) and ``area``.  Every shift keeps the lesion's bounding box inside the image; 0 is always admissible."""
    active = rng.random() < cfg["p"]
    n = rng.randint(1, cfg["max_lesions"])
    sr, sc = (None, None) if cfg["shift"] is None else cfg["shift"]
    items = []
    for _ in range(cfg["max_lesions"]):
        rec, comp, area, r0, c0, r1, c1 = (int(v) for v in bank.table[rng.randrange(len(bank.table))])
        coin = rng.random() < 0.5
        flip = int(coin and cfg["flip"])
        dr = rng.randint(*_span(-r0, H - 1 - r1, sr))
        f0, f1 = (W - 1 - c1, W - 1 - c0) if flip else (c0, c1)
        dc = rng.randint(*_span(-f0, W - 1 - f1, sc))
        items.append({"record": rec, "comp": comp, "dr": dr, "dc": dc, "flip": flip, "need": max(1, math.ceil(cfg["min_landed"] * area)),
                      "box": (r0, c0, r1, c1), "area": area})
    return {"active": active, "n": n, "items": items}


def sample_table(params: List[dict], device):
    """The device table of ``UssegPasteSample`` that ``usseg_lesion_paste`` reads on every launch -> uint8 tensor [len(params) * 168]."""
    import torch
    from . import _lib as L
    assert L.PASTE_MAX_ITEMS == MAX_ITEMS
    arr = (L.PasteSample * len(params))()
    for i, p in enumerate(params):
        s = arr[i]
        s.active, s.n_items = int(bool(p["active"])), int(p["n"])
        for q, it in enumerate(p["items"][:MAX_ITEMS]):
            d = s.items[q]
            d.record, d.comp, d.dr, d.dc, d.flip, d.need = (int(it[k]) for k in ("record", "comp", "dr", "dc", "flip", "need"))
            d.r0, d.c0, d.r1, d.c1 = (int(v) for v in it["box"])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


# ------------------------------------------------------------------------------------------------ the launch
def lesion_paste(x, y, table, x_bank, y_bank, labels_bank, protect: bool = True, counts=None, out=None, landed=None):
    """``usseg_lesion_paste`` on the current stream: x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32 (contiguous, on the device), ``table`` of
    ``sample_table``, the bank ``x_bank`` [N,H,W,C] in x's dtype, ``y_bank`` fp32 [N,H,W] and ``labels_bank`` int32 [N,H,W] -> (x_out, y_out,
    landed int32 [B,4]).  ``counts`` int64 [2] is added into (items accepted, pixels pasted; made and zeroed when None: ask for it back through
    ``landed`` alone then).  ``out``: (x_out, y_out) to write into (a captured graph's static buffers).  Nothing synchronises."""
    import torch
    from . import _lib as L
    ts = (x, y, table, x_bank, y_bank, labels_bank)
    if not all(t.is_cuda for t in ts):
        raise RuntimeError("lesion_paste runs on the GPU only: there is no CPU fallback")
    if x.dim() != 4 or y.dim() != 3 or x.dtype not in (torch.float32, torch.float64) or y.dtype != torch.float32 or tuple(y.shape) != tuple(x.shape[:3]):
        raise ValueError(f"lesion_paste: x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32, got {tuple(x.shape)} {x.dtype} and {tuple(y.shape)} {y.dtype}")
    B, H, W, Cc = x.shape
    N = x_bank.shape[0]
    if (x_bank.dtype != x.dtype or tuple(x_bank.shape) != (N, H, W, Cc) or y_bank.dtype != torch.float32 or tuple(y_bank.shape) != (N, H, W)
            or labels_bank.dtype != torch.int32 or tuple(labels_bank.shape) != (N, H, W)):
        raise ValueError(f"lesion_paste: a bank of x [N,{H},{W},{Cc}] {x.dtype}, y fp32 [N,{H},{W}] and labels int32 [N,{H},{W}], got "
                         f"{tuple(x_bank.shape)} {x_bank.dtype}, {tuple(y_bank.shape)} {y_bank.dtype}, {tuple(labels_bank.shape)} {labels_bank.dtype}")
    if not all(t.is_contiguous() for t in ts):
        raise ValueError("lesion_paste: x, y, the table and the bank must be contiguous")
    if table.numel() * table.element_size() != B * C.sizeof(L.PasteSample):
        raise ValueError(f"lesion_paste: a table of {B} samples, got {table.numel() * table.element_size()} bytes")
    lib = L.load()
    xo, yo = (torch.empty_like(x), torch.empty_like(y)) if out is None else out
    if xo.shape != x.shape or xo.dtype != x.dtype or yo.shape != y.shape or yo.dtype != y.dtype or not (xo.is_contiguous() and yo.is_contiguous()):
        raise ValueError("lesion_paste: out must match x and y in shape and dtype and be contiguous")
    if landed is None:
        landed = torch.empty((B, L.PASTE_MAX_ITEMS), dtype=torch.int32, device=x.device)
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device=x.device)
    if landed.dtype != torch.int32 or tuple(landed.shape) != (B, L.PASTE_MAX_ITEMS) or counts.dtype != torch.int64 or counts.numel() != 2 \
            or not (landed.is_contiguous() and counts.is_contiguous() and landed.is_cuda and counts.is_cuda):
        raise ValueError("lesion_paste: landed int32 [B,4] and counts int64 [2], contiguous on the device")
    d = L.PasteDesc(B, H, W, Cc, 1 if x.dtype == torch.float64 else 0, N, 1 if protect else 0)
    L.check(lib.usseg_lesion_paste(C.byref(d), table.data_ptr(), x.data_ptr(), y.data_ptr(), x_bank.data_ptr(), y_bank.data_ptr(),
                                   labels_bank.data_ptr(), xo.data_ptr(), yo.data_ptr(), landed.data_ptr(), counts.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "lesion_paste")
    return xo, yo, landed


def paste_batch(x, y, params: List[dict], cfg: dict, bank: LesionBank, x_bank, y_bank, counts=None):
    """x [B,H,W,C] fp32 / fp64 and y [B,H,W] fp32 ON THE DEVICE, ``params`` one ``draw_paste`` dict per sample -> (x_pasted, y_pasted) of the same
    shapes and dtypes.  ``counts``: the epoch's int64 [2] device counters (``lesion_paste``)."""
    if len(params) != x.shape[0]:
        raise ValueError(f"paste_batch: {len(params)} parameter sets for {x.shape[0]} samples")
    xo, yo, _ = lesion_paste(x.contiguous(), y.contiguous(), sample_table(params, x.device), x_bank, y_bank, bank.labels, protect=cfg["protect"],
                             counts=counts)
    return xo, yo


def paste_line(placed: int, drawn: int, pixels: int) -> str:
    """The drivers' line per epoch."""
    return "paste: {} of {} lesions placed, {} pixels pasted".format(placed, drawn, pixels)
