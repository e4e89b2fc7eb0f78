"""Timing of the brain-mask cascade (TBIEvaluator.Cascade: mask model -> gate -> bleed model -> maps) at 256x80x10 (diagnostic).

    python tools/time_cascade.py                 # the table: ms per call, median of --repeats runs of --calls back-to-back calls
    python tools/time_cascade.py --trace         # a few eager cascade calls at B=16 (after a warm-up), for a kernel trace:
                                                 # rocprofv3 --kernel-trace --stats -- python tools/time_cascade.py --trace

Paths per batch size (B=1 and B=16):
    host_mask_ms      mask.predict -> probabilities to the host -> np.round mask in NumPy -> upload -> bleed.predict (the reference's
                      order of work, in one process)
    cascade_eager_ms  Cascade.predict, eager
    cascade_graph_ms  Cascade.predict replaying its one captured graph
    predict_graph_ms  one model's captured predict, for scale (the graph cascade holds two of them, the gate and the maps)
One JSON line per batch size.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import timing  # noqa: E402

H, W, C = 256, 80, 10


def models(B):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    return VisionTransformer(B, (H, W), 3, in_channels=C, seed=1), VisionTransformer(B, (H, W), 2, in_channels=C, seed=2)


def per_call_ms(fn, calls, repeats):
    """(median, min, max) over `repeats` windows of `calls` back-to-back calls, after three warm-up calls: ms per call."""
    sp = timing.spread(timing.time_steps(fn, repeats, calls, warm=3), 6)
    return sp["median"], sp["min"], sp["max"]


def table(args):
    from ultrasound_modeling_amd.TBIEvaluator import Cascade
    for B in (1, 16):
        bleed, mask = models(B)
        xh = np.random.default_rng(B).standard_normal((B, H, W, C)).astype(np.float32)
        x = torch.from_numpy(xh).cuda()

        def host_mask():
            pm = mask.predict(x).cpu().numpy()
            xg = xh.copy()
            xg[np.round(pm)[..., 0] == 1] = 0.0            # TBIEvaluator.py:224-227
            return bleed.predict(xg)

        r = {"shape": [B, H, W, C], "calls": args.calls, "repeats": args.repeats}
        r["host_mask_ms"] = per_call_ms(host_mask, args.calls, args.repeats)
        cas = Cascade(bleed, mask)
        r["cascade_eager_ms"] = per_call_ms(lambda: cas.predict(x), args.calls, args.repeats)
        cas.capture_predict_graph(x)
        r["cascade_graph_ms"] = per_call_ms(lambda: cas.predict(x), args.calls, args.repeats)
        bleed.capture_predict_graph(x)
        r["predict_graph_ms"] = per_call_ms(lambda: bleed.predict(x), args.calls, args.repeats)
        print(f"B={B} {H}x{W}x{C}: host mask {r['host_mask_ms'][0]:.3f} ms, cascade eager {r['cascade_eager_ms'][0]:.3f} ms, cascade graph "
              f"{r['cascade_graph_ms'][0]:.3f} ms, one predict graph {r['predict_graph_ms'][0]:.3f} ms (median of {args.repeats} x "
              f"{args.calls} calls)", flush=True)
        print(json.dumps(r), flush=True)
        del bleed, mask, cas
        torch.cuda.empty_cache()


def trace():
    from ultrasound_modeling_amd.TBIEvaluator import Cascade
    bleed, mask = models(16)
    cas = Cascade(bleed, mask)
    x = torch.randn(16, H, W, C, device="cuda")
    for _ in range(4):            # the first is the warm-up
        cas.predict(x)
    torch.cuda.synchronize()
    print("trace: 4 eager cascade calls at [16,256,80,10]", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    trace() if a.trace else table(a)
