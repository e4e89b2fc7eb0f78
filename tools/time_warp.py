"""Times the online augmentation of one training batch without and with the elastic / affine warp inside a captured HIP graph:
``usseg_augment`` alone (what a run without ``warp=`` launches per batch) and ``usseg_elastic_warp`` followed by ``usseg_augment`` on the
warped batch, at 16 x 256 x 80 x 10 fp64 with sigma 8 (radius 32), a generated field and every sample active.  Each variant is one graph of
--reps repetitions on the same buffers, replayed --iters times; prints the median time per repetition, the addition, and the bandwidth the
addition achieves over the bytes the warp must move (x and y read and written once, the workspace written and read once), and writes the
numbers to --out.  DESIGN.md section 4h-2.

usage: python tools/time_warp.py [--reps 20] [--iters 15] [--out profiles/warp_time.json]"""
import argparse
import ctypes as C
import os
import random
import sys

import torch

import timing

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ultrasound_modeling_amd import DataAugs, _lib as L, ops, warp as Wp  # noqa: E402

SHAPE = (16, 256, 80, 10)
STEP_MS = (2.77, 2.91)          # the Arch B training step (README)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "warp_time.json"))
    a = ap.parse_args()
    timing.require_gpu("time_warp")
    B, H, W, Cc = SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(SHAPE, generator=g, device="cuda", dtype=torch.float64)
    y = torch.randint(0, 3, (B, H, W), generator=g, device="cuda").float()
    rng = random.Random(2)
    aug_table = DataAugs._sample_table([DataAugs.draw(rng) for _ in range(B)], x.device)
    cfg = Wp.warp_config(dict(p=1.0))
    warp_table = Wp.sample_table([Wp.draw_warp(rng, cfg, H, W) for _ in range(B)], x.device)
    weights = Wp.device_weights(cfg["sigma"], x.device)
    cp = ops.roundup(Cc, 8)
    xo = torch.empty((B, H, W, cp), dtype=torch.bfloat16, device="cuda")
    yv = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
    xw, yw = torch.empty_like(x), torch.empty_like(y)
    lib, desc = L.load(), L.AugDesc(B, H, W, Cc, cp, 3)

    def augment(xs, ys):
        L.check(lib.usseg_augment(C.byref(desc), aug_table.data_ptr(), xs.data_ptr(), 1, ys.data_ptr(), None, xo.data_ptr(), None, None, yv.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "augment")

    def warp_augment():
        Wp.elastic_warp(x, y, warp_table, weights, out=(xw, yw))
        augment(xw, yw)
    ts = timing.time_calls({"augment": lambda: augment(x, y), "both": warp_augment}, a.iters, a.reps, replays=1)      # the two alternate
    (aug, aug_min), (both, both_min) = ((sp["median"], sp["min"]) for sp in (timing.spread(ts["augment"]), timing.spread(ts["both"])))
    added = both - aug
    pixels = B * H * W
    nbytes = 2 * pixels * Cc * 8 + 2 * pixels * 4 + 2 * int(lib.usseg_warp_ws_bytes(B, H, W))
    result = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "dtype": "float64", "sigma": cfg["sigma"], "radius": Wp.gaussian_radius(cfg["sigma"]),
              "reps": a.reps, "iters": a.iters, "unit": "us per repetition, median of iters",
              "augment": {"median_us": round(aug, 2), "min_us": round(aug_min, 2)},
              "warp_then_augment": {"median_us": round(both, 2), "min_us": round(both_min, 2)},
              "added_us": round(added, 2), "warp_bytes": nbytes, "warp_achieved_TB_per_s": round(nbytes / (added * 1e-6) / 1e12, 3) if added > 0 else None,
              "added_over_archB_step": [round(added * 1e-3 / s, 4) for s in STEP_MS]}
    print(f"augment alone            median {aug:7.1f} us  min {aug_min:7.1f} us", flush=True)
    print(f"warp, then augment       median {both:7.1f} us  min {both_min:7.1f} us", flush=True)
    print(f"added by the warp        {added:7.1f} us = {100 * added * 1e-3 / STEP_MS[0]:.1f} % of a {STEP_MS[0]} ms step; {nbytes / 1e6:.1f} MB at "
          f"{result['warp_achieved_TB_per_s']} TB/s", flush=True)
    timing.write_json(a.out, result)


if __name__ == "__main__":
    main()
