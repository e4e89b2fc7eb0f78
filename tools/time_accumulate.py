"""Times gradient accumulation (csrc/accumulate.hip), everything replayed from HIP graphs through tools/timing.py:

  * ``usseg_grad_accumulate`` alone, both behaviours, at the flat buffer sizes of Arch B (6.27 M) and Arch A (25.7 M) beside
    ``usseg_adam_clip_step`` on buffers of the same size, the three alternating inside every round; per call the bytes it must move (the
    micro-step 12 B per parameter, the finishing launch 16 B, Adam 28 B) and the bytes/s that gives, and each accumulate launch's bytes/s over
    Adam's in the same run (expected: at least 1; below 0.8 is reported as a finding).  These are back-to-back figures: a launch finds what
    the one before it left in the 256 MB Infinity Cache, and the accumulate launches have two buffers where Adam has four, so at the Arch A
    size theirs fit the cache and Adam's do not.  The cost of the launch inside a step, with a forward / backward between two uses of the
    accumulator, is what the step timings below show;
  * one captured training step of the model at the benchmark's Arch B shape: the default step (``accumulate=None``), and with ``accumulate=4``
    a micro-step and the finishing step, each timed through ``train_step`` with the host counter of pending micro-steps set before every
    call.  With ``--parent DIR`` (a checkout of the parent commit, built there) the default step of the code that has no accumulation at all
    is timed too, the two trees alternating, one fresh process per tree and round.

usage: python tools/time_accumulate.py [--parent DIR] [--rounds N] [--replays K] [--reps R] [--iters I] [--json PATH] [B H W]
       python tools/time_accumulate.py --child ROOT [--with-accumulate] [--replays K] [B H W]      (one round of one tree: prints a JSON line)"""
import argparse
import os
import sys

import timing

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--child", default=None)
ap.add_argument("--with-accumulate", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=30)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--json", default=os.path.join(HERE, "profiles", "accumulate_step.json"))
ap.add_argument("shape", nargs="*", type=int, default=[16, 256, 256])
a = ap.parse_args()
B, H, W = a.shape
N_STEP = 4
SIZES = {"ArchB": 6_270_000, "ArchA": 25_700_000}


def child(root, with_accumulate):
    """One round of one tree -> {"default": ms per step} and, from a tree that accumulates, {"micro", "finish"} with accumulate=N_STEP."""
    sys.path.insert(0, root)
    import torch
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    x, y = timing.bleed_batch(B, H, W, 1, torch.Generator().manual_seed(0))
    net = VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1)
    net.capture_graph(x, y)
    res = {"default": timing.time_steps(lambda: net.train_step(x, y), 1, a.replays)[0]}
    del net
    if with_accumulate:
        net = VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1, accumulate=N_STEP)
        net.capture_graph(x, y)

        def at(pending):
            def step():
                net._pending = pending          # 0: the replayed step is a micro-step; N - 1: it finishes the group
                net.train_step(x, y)
            return step
        res["micro"] = timing.time_steps(at(0), 1, a.replays)[0]
        res["finish"] = timing.time_steps(at(N_STEP - 1), 1, a.replays)[0]
        net._pending = 0
    timing.emit("TIME_ACCUMULATE", res)


if a.child is not None:
    child(a.child, a.with_accumulate)
    sys.exit(0)

import torch                                                                      # noqa: E402
sys.path.insert(0, HERE)
from ultrasound_modeling_amd import ops                                           # noqa: E402

timing.require_gpu("time_accumulate")
out = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W], "accumulate": N_STEP, "kernel": {}, "step_ms": {}}
print(f"usseg_grad_accumulate beside usseg_adam_clip_step (HIP-graph replay, {a.reps} calls a graph, {a.iters} rounds, the three alternating):")
for name, n in SIZES.items():
    p, g, m, v, acc, fin_acc, fin_g = (torch.randn(n, device="cuda") * s for s in (0.1, 1e-3, 1e-4, 0.0, 0.0, 0.0, 1e-3))
    sumsq = torch.zeros(ops.ACC_FLOATS, device="cuda")
    lr_t = torch.full((1,), 1e-5, device="cuda")
    variants = {
        "adam_clip_step": (28, lambda: ops.adam_clip_step(p, g, m, v, sumsq, 0.0, lr_t, 0.9, 0.999, 1e-7)),
        "grad_accumulate, micro-step": (12, lambda: ops.grad_accumulate(acc, g, False, float(N_STEP))),
        # buffers of its own: it rewrites both.  From a zero accumulator and with divisor 1 a call leaves fin_g = (0 + fin_g) / 1 = fin_g, so
        # every one of the calls works on the same nonzero data (dividing by N would halve the exponents call by call down to zeros); the
        # launch is the same - the divisor is a kernel argument and the division sequence does not depend on its value
        "grad_accumulate, finish": (16, lambda: ops.grad_accumulate(fin_acc, fin_g, True, 1.0)),
    }
    ts = timing.time_calls({k: fn for k, (_, fn) in variants.items()}, a.iters, a.reps, replays=1)
    row = {"n": n}
    for label, (nbytes, _) in variants.items():
        sp = timing.spread(ts[label], 2)
        row[label] = dict(sp, bytes_per_parameter=nbytes, TB_per_s=round(n * nbytes / sp["median"] / 1e6, 3))
        print(f"  {name} n={n} {label:28s} {sp['min']:7.2f} us min, {sp['median']:7.2f} median, {sp['max']:7.2f} max   {nbytes} B/parameter -> "
              f"{row[label]['TB_per_s']:.2f} TB/s", flush=True)
    for label in ("grad_accumulate, micro-step", "grad_accumulate, finish"):
        r = row[label]["TB_per_s"] / row["adam_clip_step"]["TB_per_s"]
        row[label]["bytes_per_s_over_adam"] = round(r, 3)
        print(f"  {name}: {label}: {r:.2f}x the bytes/s of adam_clip_step" + ("" if r >= 0.8 else "   <-- below 0.8: a finding, not the expectation"), flush=True)
    out["kernel"][name] = row
    del p, g, m, v, acc, fin_acc, fin_g, variants

trees = [("this", HERE, ["--with-accumulate"])] + ([("parent", os.path.abspath(a.parent), [])] if a.parent else [])
print(f"Arch B {B} x {H} x {W} x 1 training step, HIP-graph replay, {a.rounds} rounds of {a.replays} replays, the trees alternating:")
runs = timing.alternate_trees(os.path.abspath(__file__), trees, a.rounds, "TIME_ACCUMULATE", ["--replays", str(a.replays), str(B), str(H), str(W)], timeout=600)
for key, ts in runs.items():
    sp = timing.spread(ts)
    out["step_ms"][key] = dict(sp, rounds=[round(t, 4) for t in ts])
    print(f"  step, {key:16s} {sp['min']:8.4f} ms min, {sp['median']:8.4f} median, {sp['max']:8.4f} max", flush=True)
med = {k: s["median"] for k, s in out["step_ms"].items()}
out["micro_over_default"] = round(med["this:micro"] / med["this:default"], 4)
out["finish_over_default"] = round(med["this:finish"] / med["this:default"], 4)
out["group_of_%d_over_%d_default_steps" % (N_STEP, N_STEP)] = round(((N_STEP - 1) * med["this:micro"] + med["this:finish"]) / (N_STEP * med["this:default"]), 4)
print(f"  micro-step / default step = {out['micro_over_default']:.3f}; finishing step / default step = {out['finish_over_default']:.3f}")
if "parent:default" in med:
    out["default_over_parent"] = round(med["this:default"] / med["parent:default"], 4)
    print(f"  default step / the parent commit's = {out['default_over_parent']:.4f} (the README's box spread: +-4 %)")
timing.write_json(a.json, out)
