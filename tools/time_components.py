"""Timing of connected-component labelling and mask clean-up (csrc/components.hip; diagnostic).

    python tools/time_components.py

`label_components` and `clean_mask` (min_area 5, with the probability map and min_peak 0.6) are captured in a HIP graph each; a round is three
replays between two events, the figure the median of five rounds, in microseconds per call.  Shapes 16 x 256 x 80 and 16 x 256 x 256, inputs
    model     bleed_prob > 0.5 of a randomly initialised model on random input (speckle)
    blob      one disc per image
    random    random pixels at density 0.59 (4-connectivity: near the percolation threshold, the longest winding components)
Beside each: the path this replaces - the mask copied to the host and scipy.ndimage.label per image, one process - as the median of five.
One JSON line per (shape, input, connectivity).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import timing  # noqa: E402

from ultrasound_modeling_amd import ops  # noqa: E402

N, REPLAYS, ROUNDS = 16, 3, 5
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


def triple(ts):
    sp = timing.spread(ts, 1)
    return [sp["median"], sp["min"], sp["max"]]


def scipy_us(mask, connectivity):
    """the host path: copy the mask to the host, scipy.ndimage.label per image"""
    from scipy import ndimage as nd
    out, k = [], 0
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = mask.cpu().numpy()
        k = sum(nd.label(p, structure=STRUCTURE[connectivity])[1] for p in m)
        out.append((time.perf_counter() - t0) * 1e6)
    return triple(out), k


def inputs(H, W):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    model = VisionTransformer(N, (H, W), 3, in_channels=10, seed=1)
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((N, H, W, 10)).astype(np.float32)).cuda()
    _, bleed_prob = ops.cascade_maps(model.predict(x))
    bleed_prob = bleed_prob.clone()
    del model
    torch.cuda.empty_cache()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blob = ((yy - H // 3) ** 2 + (xx - W // 2) ** 2 <= (min(H, W) // 6) ** 2)
    rnd = torch.from_numpy(np.random.default_rng(3).random((N, H, W)) < 0.59)
    prob = torch.rand((N, H, W), generator=torch.Generator().manual_seed(4)).cuda()
    return (("model", (bleed_prob > 0.5).to(torch.uint8), bleed_prob),
            ("blob", blob.to(torch.uint8).expand(N, H, W).contiguous().cuda(), prob),
            ("random", rnd.to(torch.uint8).cuda(), prob))


def main():
    timing.require_gpu("time_components")
    for H, W in ((256, 80), (256, 256)):
        ws = torch.empty(ops.components_ws_bytes(N, H, W), dtype=torch.uint8, device="cuda")
        labels = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
        count = torch.empty((N,), dtype=torch.int32, device="cuda")
        for name, mask, prob in inputs(H, W):
            out = torch.empty_like(mask)
            for c in (4, 8):
                r = {"shape": [N, H, W], "input": name, "connectivity": c, "density": round(float(mask.float().mean()), 4)}
                ts = timing.time_calls({"label_us": lambda: ops.label_components(mask, c, labels=labels, count=count, ws=ws),
                                        "clean_us": lambda: ops.clean_mask(mask, prob, connectivity=c, min_area=5, min_peak=0.6, out=out, ws=ws)}, ROUNDS, 1, REPLAYS)
                r["label_us"] = triple(ts["label_us"])
                r["components"] = int(count.sum())
                r["clean_us"] = triple(ts["clean_us"])
                r["kept"] = round(float(out.float().mean()), 4)
                r["scipy_us"], k = scipy_us(mask, c)
                assert k == r["components"], (k, r["components"])
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
