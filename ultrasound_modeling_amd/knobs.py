"""Every USSEG_* environment switch the Python side reads: one table line each, read through ``get()`` and nowhere else.

``get(name)`` reads ``os.environ`` WHEN CALLED and raises ``KeyError`` on a name that is not in the table.  The modules call it where
they always read their switches: at import, into their module globals, or at construction time (``USSEG_QUAD_HEAD`` / ``USSEG_QUAD_TCONV``).
The switches of the kernel library are in ``csrc/knobs.h``; DESIGN.md section 4d documents both tables.

Parse rules:
  flag    unset -> bool(default); set -> value != "0"
  int     unset -> default; set -> int(value)
  optint  unset -> None ("let the caller decide"); set -> int(value)
  str     unset -> default (None: no default); set -> the value
"""
from __future__ import annotations

import os

# name: (rule, default, meaning)
KNOBS = {
    "USSEG_LIB":                ("str",    None,  "path of a diagnostic build of the same sources to load instead of the in-tree library"),
    "USSEG_SIDE_STREAM":        ("flag",   0,     "weight gradients fork to a side stream per launch inside an overlap region"),
    "USSEG_DEFER":              ("flag",   1,     "defer the finishing reductions to the end of the region (0: finish after each producer)"),
    "USSEG_LAZY_WGRAD":         ("flag",   1,     "lazy weight gradients: queued and run on the side stream beside the backward-data chain"),
    "USSEG_FUSE_LN_RES":        ("flag",   1,     "LayerNorm backward + residual add in one pass (transformer blocks)"),
    "USSEG_ENC_LAZY":           ("optint", None,  "bit mask of the ResNest stages whose weight gradients are lazy (unset: 12, or 0 in front of a ViT)"),
    "USSEG_FOLD_BN":            ("flag",   1,     "inference BatchNorm folded into the producing conv's packed weights"),
    "USSEG_FUSED_CARDINAL":     ("flag",   1,     "cardinal group + shortcut of a stage as one launch"),
    "USSEG_FUSED_CARDINAL_BWD": ("flag",   1,     "its backward chain + the shortcut norm's backward as one launch"),
    "USSEG_CARD_BWD_MAX_PX":    ("int",    32768, "most pixels of a stage for the fused cardinal backward"),
    "USSEG_LN_PAIR":            ("flag",   1,     "shortcut norm backward + conv2_bn backward of the large stages in one launch"),
    "USSEG_FUSED_STEM_BWD":     ("flag",   1,     "stem backward-data fused with the norm / activation backward in front"),
    "USSEG_STEM_WGRAD_MERGE":   ("flag",   1,     "the stem's three weight gradients in one multi-job launch"),
    "USSEG_FUSED_STEM":         ("flag",   1,     "the stem (three convs, two norms, pool) as one launch"),
    "USSEG_MERGED_DGRAD":       ("flag",   1,     "one backward-data GEMM for a stage's grouped 1x1 and shortcut 1x1"),
    "USSEG_FUSED_DGRAD":        ("flag",   1,     "the DecoderBlock's four branch backward-data passes as one launch"),
    "USSEG_BRANCH4":            ("flag",   1,     "the DecoderBlock's 1x1 branch as a fourth job of the dilated branches' launch"),
    "USSEG_QUAD_UP":            ("flag",   0,     "the decoder's transposed convs in quad (parity-class) form"),
    "USSEG_QUAD_HEAD":          ("flag",   1,     "the <= 4-class head's transposed conv in quad form (read at construction)"),
    "USSEG_QUAD_TCONV":         ("flag",   0,     "Arch A's inner transposed convs in quad form (read at construction)"),
    "USSEG_STAGE_LAZY":         ("flag",   1,     "Arch A: per-stage lazy weight gradients"),
    "USSEG_FUSED_HEAD":         ("flag",   1,     "head conv + softmax + loss as one launch"),
    "USSEG_VIT_LAZY":           ("str",    "enc", "lazy weight gradients of the ViT: whole encoder (enc), per block (block), or 0"),
    "USSEG_FUSED_ATTN":         ("flag",   1,     "train-step attention on the fused kernels (head size 128)"),
    "USSEG_SWIN_LAZY":          ("flag",   1,     "Swin: per-block lazy weight gradients"),
    "USSEG_DIST_BACKEND":       ("str",    None,  "torch.distributed backend (unset: nccl with a GPU, else gloo)"),
    "USSEG_DP_CHUNKS":          ("int",    0,     "chunks of the pipelined gradient exchange (0 or 1: one exchange)"),
}


def get(name: str):
    rule, default, _ = KNOBS[name]
    v = os.environ.get(name)
    if rule == "flag":
        return bool(default) if v is None else v != "0"
    if v is None:
        return default
    return v if rule == "str" else int(v)
