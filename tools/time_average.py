"""Times the AdamW update without an average (usseg_adamw_step), the update fused with the EMA / SWA average (usseg_adamw_avg_step), and
the two-launch path (usseg_adamw_step then usseg_average_update) inside a captured HIP graph, at the flat buffer sizes of Arch B (6.27 M)
and Arch A (25.7 M).  Each variant is one graph of --reps repetitions on the same buffers, replayed --iters times; prints the median time
per repetition beside the HBM bound at 6.29 TB/s (28 B per parameter for the update, 36 B fused, 28 + 12 B for the two launches) and writes
the numbers to --out.  The fused launch blends at every step here (EMA: the full 36 B); "fused, no snapshot" is an SWA step between two
snapshots (c = 0: avg is neither read nor written).  DESIGN.md section 4g-2.

usage: python tools/time_average.py [--reps 20] [--iters 15] [--out profiles/average_step.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ultrasound_modeling_amd import flat, ops  # noqa: E402

SIZES = {"ArchB": 6_270_000, "ArchA": 25_700_000}
HBM = 6.29e12
HYPER = (0.9, 0.999, 1e-7)


def _time(fn, reps, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "average_step.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters, "unit": "us per repetition, median of iters", "sizes": {}}
    for name, n in SIZES.items():
        p, g, m, v = (torch.randn(n, device="cuda") * s for s in (0.1, 1e-3, 1e-4, 0.0))
        v.abs_()
        avg = p.clone()
        sumsq = torch.zeros(ops.ACC_FLOATS, device="cuda")
        lr_t = torch.full((1,), 1e-5, device="cuda")
        wd = torch.full((1,), 1e-6, device="cuda")
        step = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        ema = torch.from_numpy(flat._average_words(flat.average_config({"mode": "ema", "decay": 0.999}))).cuda()
        swa = torch.from_numpy(flat._average_words(flat.average_config({"mode": "swa", "start": 5, "period": 1000}))).cuda()

        def two():
            ops.adamw_step(p, g, m, v, sumsq, 0.0, lr_t, wd, None, *HYPER)
            ops.average_update(avg, p, step, ema)
        variants = {
            "adamw_step": (28, lambda: ops.adamw_step(p, g, m, v, sumsq, 0.0, lr_t, wd, None, *HYPER)),
            "fused": (36, lambda: ops.adamw_avg_step(p, g, m, v, avg, sumsq, 0.0, lr_t, wd, None, *HYPER, step, ema)),
            "adamw_step + average_update": (40, two),
            "fused, no snapshot": (28, lambda: ops.adamw_avg_step(p, g, m, v, avg, sumsq, 0.0, lr_t, wd, None, *HYPER, step, swa)),
        }
        row = {"n": n}
        for label, (nbytes, fn) in variants.items():
            med, lo = _time(fn, a.reps, a.iters)
            bound = n * nbytes / HBM * 1e6
            row[label] = {"median_us": round(med, 2), "min_us": round(lo, 2), "hbm_bound_us": round(bound, 2)}
            print(f"{name} n={n} {label:28s} median {med:7.1f} us  min {lo:7.1f} us  (HBM bound {bound:6.1f} us)", flush=True)
        base, fused, pair = (row[k]["median_us"] for k in ("adamw_step", "fused", "adamw_step + average_update"))
        row["fused_over_adamw_step"] = round(fused / base, 4)
        row["bound_9_7_x_1_10"] = round(9 / 7 * 1.10, 4)
        row["fused_within_bound"] = fused <= base * 9 / 7 * 1.10
        row["fused_not_slower_than_two_launches"] = fused <= pair
        print(f"{name}: fused / adamw_step = {fused / base:.3f} (bound {9 / 7 * 1.10:.3f}); two launches / fused = {pair / fused:.3f}", flush=True)
        result["sizes"][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
