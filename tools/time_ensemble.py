"""Times ensemble prediction (csrc/ensemble.hip, ultrasound_modeling_amd/ensemble.py) at the evaluator's shape, everything replayed from HIP
graphs as tools/time_lovasz.py does:

  * the merge launch alone for every K given: `reps` launches per graph, `rounds` graphs, the median beside the bytes the launch must move
    ((K*C + C + 2 + C) * 4 per pixel: every member read once, every output written once) and their ratio; likewise the image-scores launch
    and one calibration launch;
  * the captured ``Ensemble.predict`` of K Arch B members (K/2 seeded models, each with its left-right mirror) against K back-to-back replays
    of ONE model's own predict graph in the same process - the cost of K predictions as the project stands - alternating the two within every
    round.  The ensemble adds one mirror copy of the input, the merge and the image-scores launch to those K predictions.

usage: python tools/time_ensemble.py [--k K ...] [--rounds N] [--replays R] [--reps R] [--no-models] [--json PATH] [B H W]"""
import argparse
import os
import sys

import torch

import timing

ap = argparse.ArgumentParser()
ap.add_argument("--k", nargs="*", type=int, default=[2, 4, 8])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--replays", type=int, default=20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-models", action="store_true", help="time the launches only")
ap.add_argument("--json", default=None)
ap.add_argument("shape", nargs="*", type=int, default=[16, 256, 80])
a = ap.parse_args()
B, H, W = a.shape
C_ = 3
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ultrasound_modeling_amd import ops                                         # noqa: E402

timing.require_gpu("time_ensemble")
out = {"shape": [B, H, W, C_], "launch_us": {}, "predict_ms": {}}
g = torch.Generator().manual_seed(0)
M = B * H * W


def rows(named):
    """Time the named launches (name -> (fn, bytes)), three replays a window, alternating inside every round."""
    ts = timing.time_calls({n: fn for n, (fn, _) in named.items()}, a.rounds, a.reps, replays=3)
    for name, (_, nbytes) in named.items():
        s = timing.spread(ts[name])
        out["launch_us"][name] = dict(s, MB=round(nbytes / 1e6, 2), TBps=round(nbytes / s["median"] / 1e6, 3))
        print(f"  {name:34s} {s['min']:8.2f} us min, {s['median']:8.2f} median, {s['max']:8.2f} max   {nbytes / 1e6:6.2f} MB -> "
              f"{nbytes / s['median'] / 1e6:5.2f} TB/s", flush=True)


print(f"the launches at {B} x {H} x {W} x {C_} ({M} pixels), {a.rounds} graphs of {a.reps} launches:")
members = [torch.softmax(2 * torch.randn(B, H, W, C_, generator=g), -1).cuda() for _ in range(max(a.k))]
y = torch.nn.functional.one_hot(torch.randint(0, C_, (B, H, W), generator=g), C_).float().cuda()
bufs = dict(mean_probs=torch.empty_like(members[0]), entropy=torch.empty(B, H, W).cuda(), mutual_info=torch.empty(B, H, W).cuda(),
            variance_out=torch.empty_like(members[0]))
named = {}
for K in a.k:
    flip_w = 0xAAAA & ((1 << K) - 1)                                             # every second member mirrored, as Ensemble(flip=True) orders them
    named[f"ensemble_merge K={K} (mirrored {bin(flip_w).count('1')})"] = (lambda K=K, flip_w=flip_w: ops.ensemble_merge(members[:K], flip_w, **bufs), (K * C_ + C_ + 2 + C_) * 4 * M)
    named[f"ensemble_merge K={K} (none mirrored)"] = (lambda K=K: ops.ensemble_merge(members[:K], 0, **bufs), (K * C_ + C_ + 2 + C_) * 4 * M)
scores, counts = torch.empty(B, 4).cuda(), torch.empty(B, dtype=torch.int32).cuda()
named["ensemble_image_scores"] = (lambda: ops.ensemble_image_scores(bufs["mean_probs"], bufs["entropy"], bufs["mutual_info"], scores, counts), (C_ + 2) * 4 * M)
cal = torch.zeros(15 * 3 + 2, dtype=torch.int64).cuda()
named["calibration_bins, 15 bins, top label"] = (lambda: ops.calibration_bins(members[0], y, cal, 15, -1), 2 * C_ * 4 * M)
rows(named)

if not a.no_models:
    from ultrasound_modeling_amd.ensemble import Ensemble                        # noqa: E402
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer     # noqa: E402
    x = torch.randn(B, H, W, 10, generator=g).clamp_(-1, 1).cuda()
    models = [VisionTransformer(B, (H, W), C_, in_channels=10, seed=3 + i) for i in range(max(1, max(a.k) // 2))]
    single = models[0]
    single.capture_predict_graph(x)
    sx = single.predict_inputs()

    print(f"Arch B {B} x {H} x {W} x 10, captured predict, {a.rounds} rounds of {a.replays} replays, the two forms alternating:")
    for K in a.k:
        if K % 2:
            print(f"  K={K}: skipped (members come in mirror pairs)")
            continue
        ens = Ensemble(models[:K // 2], flip=True)
        ens.capture_predict_graph(x)
        ex = ens.predict_inputs()

        def k_singles():
            for _ in range(K):
                single.predict(sx)

        forms = {"singles": k_singles, "ensemble": lambda: ens.predict(ex)}
        ts = {n: [] for n in forms}
        for r, n in timing.schedule(list(forms), a.rounds):                     # one window of each form per round; the first round warms up
            ts[n] += timing.time_steps(forms[n], 1, a.replays, warm=0 if r else 3)
        se, ss = timing.spread(ts["ensemble"]), timing.spread(ts["singles"])
        out["predict_ms"][str(K)] = {"ensemble": se, "k_single_replays": ss, "ratio_of_medians": round(se["median"] / ss["median"], 4)}
        print(f"  K={K}: ensemble graph {se['min']:8.4f} ms min, {se['median']:8.4f} median, {se['max']:8.4f} max | {K} single replays "
              f"{ss['min']:8.4f} min, {ss['median']:8.4f} median, {ss['max']:8.4f} max | ensemble / singles = {se['median'] / ss['median']:.4f}", flush=True)
        del ens

if a.json:
    timing.write_json(a.json, out)
