"""Plain NumPy restatement of the lesion copy-paste (include/usseg_paste.h) in loops after its definitions, the lesion bank
through ``scipy.ndimage.label``, and the hand-built cases that tests/test_cpu_paste.py and tests/test_gpu_paste.py share.

The fixtures are built by hand so that their properties hold by construction.  Base case, H x W = 12 x 9: labels 1.0 except row 0 and column 0,
which are 0 (outside brain).  Record 0: a 3 x 4 block of 2.0 at rows 2..4, cols 1..4, and one soft pixel of 1.5 at (11, 8).  Record 1: an L,
column 1 over rows 1..4 at 2.0 and row 4 over cols 1..3 at 1.2.  Record 2: no lesion.  With SciPy at connectivity 8 records 0 / 1 / 2 have 2 / 1 /
0 components of areas [12, 1], [6] and [].  ``layout(H, W)`` is this layout with rows scaled by kr = H // 12 and columns by kc = max(1, W // 9)
(the block's columns end at the image's last column when the image is narrower than nine)."""
import functools
import math

import numpy as np

from ultrasound_modeling_amd import _lib

MAX_ITEMS = _lib.PASTE_MAX_ITEMS                                   # the header's USSEG_PASTE_MAX_ITEMS: one definition
SHAPES = [(12, 9, 2), (37, 19, 3), (16, 5, 1), (64, 80, 10)]       # (H, W, C)
F95, F105 = np.float32(0.95), np.float32(1.05)


# ------------------------------------------------------------------------------------------------ the bank
def bank_of(y_tr, connectivity=8, min_area=1):
    """-> (labels int32 [N,H,W], table int64 [L,7] of (record, comp, area, r0, c0, r1, c1)): the components of ``y_tr >= 1.05`` per record in
    SciPy's numbering, and those of at least ``min_area`` pixels, record-major then by component id."""
    from scipy import ndimage
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    labels = np.zeros(y_tr.shape, np.int32)
    rows = []
    for n in range(y_tr.shape[0]):
        lab, k = ndimage.label(y_tr[n] >= F105, structure=structure)
        labels[n] = lab
        for comp in range(1, k + 1):
            rr, cc = np.nonzero(lab == comp)
            if len(rr) >= min_area:
                rows.append((n, comp, len(rr), rr.min(), cc.min(), rr.max(), cc.max()))
    return labels, np.array(rows, np.int64).reshape(-1, 7)


# ------------------------------------------------------------------------------------------------ the paste
def _exists(it, N):
    return 0 <= it["record"] < N and it["comp"] >= 1


def _donor(it, r, c, H, W):
    """The donor pixel of target (r, c), or None when it lies outside the image or outside the item's box."""
    pr, cf = r - it["dr"], c - it["dc"]
    pc = W - 1 - cf if it["flip"] else cf
    r0, c0, r1, c1 = it["box"]
    if not (0 <= pr < H and 0 <= pc < W and r0 <= pr <= r1 and c0 <= pc <= c1):
        return None
    return pr, pc


def _ok(yv, protect):
    return bool(yv > F95) and not (protect and bool(yv >= F105))      # a NaN compares false


def decide(y, samples, labels, protect):
    """The decisions of one call -> dict: ``src`` int64 [B,H,W] (the bank pixel record*H*W + r*W + c that a pixel comes from, -1: its own),
    ``landed`` int32 [B,4], ``counts`` int64 [2] (items accepted, pixels pasted) and what the vacuity checks ask: ``rejected`` items,
    ``overwritten`` pixels (a later accepted item replaced an earlier one's), ``refused`` lesion pixels (member but not ok)."""
    B, H, W = y.shape
    N = labels.shape[0]
    src = np.full((B, H, W), -1, np.int64)
    landed = np.zeros((B, MAX_ITEMS), np.int32)
    accepted = rejected = overwritten = refused = 0
    for b, s in enumerate(samples):
        if not s["active"]:
            continue
        n = min(max(int(s["n"]), 0), MAX_ITEMS)
        for i in range(n):
            it = s["items"][i]
            if not _exists(it, N):
                continue
            hits = []
            for r in range(H):
                for c in range(W):
                    p = _donor(it, r, c, H, W)
                    if p is None or labels[it["record"], p[0], p[1]] != it["comp"]:
                        continue
                    if _ok(y[b, r, c], protect):
                        hits.append((r, c, p))
                    else:
                        refused += 1
            landed[b, i] = len(hits)
            if len(hits) >= max(it["need"], 1):
                accepted += 1
                for r, c, p in hits:
                    overwritten += src[b, r, c] >= 0
                    src[b, r, c] = (it["record"] * H + p[0]) * W + p[1]
            else:
                rejected += 1
    return {"src": src, "landed": landed, "counts": np.array([accepted, int((src >= 0).sum())], np.int64), "rejected": rejected,
            "overwritten": int(overwritten), "refused": refused}


def apply(x, y, src, x_bank, y_bank):
    """x_out, y_out of ``decide``'s ``src``: copies, element by element."""
    B, H, W, C = x.shape
    xo, yo = x.copy(), y.copy()
    xb, yb = x_bank.reshape(-1, C), y_bank.reshape(-1)
    for b, r, c in zip(*np.nonzero(src >= 0)):
        xo[b, r, c, :] = xb[src[b, r, c], :]
        yo[b, r, c] = yb[src[b, r, c]]
    return xo, yo


def paste(x, y, samples, x_bank, y_bank, labels, protect):
    """-> (x_out, y_out, landed, counts, the ``decide`` dict)."""
    d = decide(y, samples, labels, protect)
    xo, yo = apply(x, y, d["src"], x_bank, y_bank)
    return xo, yo, d["landed"], d["counts"], d


# ------------------------------------------------------------------------------------------------ the fixtures
def layout(H, W):
    """y_tr fp32 [3,H,W] of the module docstring."""
    kr, kc = H // 12, max(1, W // 9)
    assert kr >= 1 and W >= 5
    y = np.ones((3, H, W), np.float32)
    y[:, 0, :] = 0
    y[:, :, 0] = 0
    y[0, 2 * kr:5 * kr, 1:min(4 * kc, W - 1) + 1] = 2.0
    y[0, H - 1, W - 1] = 1.5
    y[1, 4 * kr:5 * kr, 1:3 * kc + 1] = 1.2
    y[1, kr:5 * kr, 1:kc + 1] = 2.0
    return y


def _nan(dtype, payload):
    if dtype == np.float32:
        return np.array([0x7FC00000 | payload], np.int32).view(np.float32)[0]
    return np.array([0x7FF8000000000000 | payload], np.int64).view(np.float64)[0]


def item(lesion, dr=0, dc=0, flip=0, need=None, min_landed=0.5):
    """An item of the bank's table row ``lesion``; ``need`` defaults to max(1, ceil(min_landed * area))."""
    rec, comp, area, r0, c0, r1, c1 = (int(v) for v in lesion)
    return {"record": rec, "comp": comp, "dr": int(dr), "dc": int(dc), "flip": int(flip), "need": max(1, math.ceil(min_landed * area)) if need is None else need,
            "box": (r0, c0, r1, c1), "area": area}


def raw_item(record, comp, H, W, need=1):
    """An item that names no lesion of the bank (a bad record or component id), its box the whole image."""
    return {"record": record, "comp": comp, "dr": 0, "dc": 0, "flip": 0, "need": need, "box": (0, 0, H - 1, W - 1), "area": 0}


@functools.lru_cache(maxsize=None)
def case(shape, dtype):
    """-> dict: the bank (``x_bank`` [3,H,W,C], ``y_bank``, ``labels``, ``table`` with min_area 1), six recipients (``x``, ``y``) and two
    hand-written sample tables (``tables``).  Recipient 1 has bleed of its own under the paste, recipient 3 a NaN label there, recipient 5 is
    inactive in the first table and holds a NaN with a payload, an Inf and -0.0; a NaN with a payload sits inside the donor block."""
    H, W, C = shape
    dtype = np.dtype(dtype).type
    kr, kc = H // 12, max(1, W // 9)
    rng = np.random.default_rng(H * 100 + W)
    y_bank = layout(H, W)
    x_bank = rng.standard_normal((3, H, W, C)).astype(dtype)
    x_bank[0, 2 * kr, 1, 0] = _nan(dtype, 0x4321)                   # inside the block of record 0
    labels, table = bank_of(y_bank, 8, 1)
    A, S, Lz = table[0], table[1], table[2]                          # the block, the soft pixel, the L
    assert tuple(A[:2]) == (0, 1) and tuple(S[:2]) == (0, 2) and S[2] == 1 and tuple(Lz[:2]) == (1, 1) and len(table) == 3
    B = 6
    x = rng.standard_normal((B, H, W, C)).astype(dtype)
    y = np.ones((B, H, W), np.float32)
    y[:, 0, :] = 0
    y[:, :, 0] = 0
    y[1, 3 * kr:4 * kr, 1:3] = 2.0                                   # its own bleed, under the block pasted kr rows down
    y[3, 3 * kr + 1, 2] = np.array([0x7FC00077], np.int32).view(np.float32)[0]
    x[5, 1, 2, 0], x[5, H - 1, W - 1, C - 1], x[5, 0, 0, 0] = _nan(dtype, 0x1234), np.inf, -0.0
    l_left = 1 - (W - 1 - 3 * kc)                                    # the flipped L moved back to columns 1..3kc
    t0 = [
        # the block kr rows down, then the flipped L over rows kr..5kr-1: both land whole, and the L's foot overwrites the block's rows 4kr..5kr-1
        {"active": 1, "n": 2, "items": [item(A, dr=kr), item(Lz, dc=l_left, flip=1)]},
        # onto the recipient's own bleed: protect refuses those pixels, the rest still reaches the need
        {"active": 1, "n": 1, "items": [item(A, dr=kr)]},
        # across the zero row: its first row fails ok, the rest is enough; then the L across the zero row and column with need = its area: rejected
        {"active": 1, "n": 2, "items": [item(A, dr=-2 * kr), item(Lz, dr=-kr, dc=-1, need=int(Lz[2]))]},
        # a NaN label under the paste, and three items that do not exist
        {"active": 1, "n": 4, "items": [item(A, dr=kr), raw_item(3, 1, H, W), raw_item(0, 0, H, W), raw_item(-1, 1, H, W)]},
        {"active": 1, "n": 0, "items": [item(A, dr=kr)]},
        {"active": 0, "n": 2, "items": [item(A, dr=kr), item(Lz)]},
    ]
    t1 = [
        {"active": 0, "n": 1, "items": [item(A)]},
        # n_items beyond the limit: four items exist.  The soft pixel to (1, 1), the block mirrored in place, the L kr rows down, the block 2kr down
        {"active": 1, "n": 7, "items": [item(S, dr=-(H - 2), dc=-(W - 2)), item(A, flip=1), item(Lz, dr=kr), item(A, dr=2 * kr)]},
        {"active": 1, "n": -3, "items": [item(A, dr=kr)]},
        {"active": 1, "n": 1, "items": [item(A, dr=kr, dc=int(A[4]) - (W - 1 - int(A[6])), flip=1)]},
        {"active": 1, "n": 2, "items": [item(Lz, flip=1, need=int(Lz[2])), item(Lz, dr=-kr, need=int(Lz[2]))]},
        {"active": 1, "n": 1, "items": [item(Lz, dr=2 * kr)]},
    ]
    return {"x": x, "y": y, "x_bank": x_bank, "y_bank": y_bank, "labels": labels, "table": table, "tables": (t0, t1), "kr": kr, "kc": kc}


@functools.lru_cache(maxsize=None)
def decided(shape, which, protect):
    """``decide`` of table ``which`` of the shape (the decisions do not depend on the dtype of x)."""
    c = case(shape, np.float32)
    return decide(c["y"], c["tables"][which], c["labels"], protect)


def restated(shape, dtype, which, protect):
    """-> (x_out, y_out, landed, counts, the ``decide`` dict) of table ``which``."""
    c, d = case(shape, dtype), decided(shape, which, protect)
    xo, yo = apply(c["x"], c["y"], d["src"], c["x_bank"], c["y_bank"])
    return xo, yo, d["landed"], d["counts"], d
