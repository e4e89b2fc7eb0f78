"""Times the fixed-rate Adam update (usseg_adam_clip_step) against the AdamW update of the schedule path (usseg_adamw_step) inside
a captured HIP graph, at the flat buffer sizes of Arch B (6.27 M) and Arch A (25.7 M): wd = 0, wd > 0, and wd > 0 with a decay mask.
Each variant is one graph of --reps launches on the same p / g / m / v buffers, replayed --iters times; prints the median time per
launch and the HBM bound of 28 B per parameter (29 with the mask) at 6.29 TB/s.  DESIGN.md section 4g.

usage: python tools/time_optim.py [--reps 20] [--iters 15]"""
import argparse
import os
import sys

import torch

import timing

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ultrasound_modeling_amd import ops  # noqa: E402

SIZES = {"ArchB": 6_270_000, "ArchA": 25_700_000}
HBM = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=15)
    a = ap.parse_args()
    for name, n in SIZES.items():
        p, g, m, v = (torch.randn(n, device="cuda") * s for s in (0.1, 1e-3, 1e-4, 0.0))
        v.abs_()
        sumsq = torch.zeros(ops.ACC_FLOATS, device="cuda")
        lr_t = torch.full((1,), 1e-5, device="cuda")
        wd0, wd = torch.zeros(1, device="cuda"), torch.full((1,), 1e-6, device="cuda")
        mask = (torch.rand(n, device="cuda") > 0.1).to(torch.uint8)
        variants = {
            "adam_clip_step": lambda: ops.adam_clip_step(p, g, m, v, sumsq, 0.0, lr_t, 0.9, 0.999, 1e-7),
            "adamw wd=0": lambda: ops.adamw_step(p, g, m, v, sumsq, 0.0, lr_t, wd0, None, 0.9, 0.999, 1e-7),
            "adamw wd>0": lambda: ops.adamw_step(p, g, m, v, sumsq, 0.0, lr_t, wd, None, 0.9, 0.999, 1e-7),
            "adamw wd>0 mask": lambda: ops.adamw_step(p, g, m, v, sumsq, 0.0, lr_t, wd, mask, 0.9, 0.999, 1e-7),
        }
        for label, ts in timing.time_calls(variants, a.iters, a.reps, replays=1).items():                           # the variants alternate
            sp = timing.spread(ts)
            bound = n * (29 if "mask" in label else 28) / HBM * 1e6
            print(f"{name} n={n} {label:16s} median {sp['median']:7.1f} us  min {sp['min']:7.1f} us  (HBM bound {bound:6.1f} us)", flush=True)


if __name__ == "__main__":
    main()
