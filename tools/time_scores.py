"""Times the score kernels (csrc/scores.hip, include/usseg_scores.h) at a test run's shape, 1024 images of 256 x 80, everything replayed from
HIP graphs as tools/time_sweep.py does: `reps` launches per graph, `rounds` graphs, the median (min - max) beside the bytes each call must move.

  * ``image_confusion`` at C = 2 without and with the area weights, and at C = 4 with them;
  * ``component_measure`` on the labels of a bleed-like stack (one or two discs per image plus 1 % speckle), at cap = the largest count;
  * ``bootstrap_sums`` at K = 8: 1000 and 10000 replicates of the 1024 images, and 10000 replicates of 64 patients (the cluster bootstrap).

Before anything is timed each result is compared with a torch expression of the same integers on the device (sums of one-hot products), so a
wrong kernel is not timed.  Nothing has a predecessor to be compared with: the numbers are a first record, not a claim.

usage: python tools/time_scores.py [--rounds N] [--reps R] [--replays P] [--json PATH] [N H W]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--replays", type=int, default=5)
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "scores_time.json"))
ap.add_argument("shape", nargs="*", type=int, default=[1024, 256, 80])
a = ap.parse_args()

import numpy as np                                                               # noqa: E402
import torch                                                                     # noqa: E402

import timing                                                                    # noqa: E402

sys.path.insert(0, ROOT)
from ultrasound_modeling_amd import ops                                          # noqa: E402
from ultrasound_modeling_amd.metrics import ScanGeometry                         # noqa: E402

timing.require_gpu("time_scores")

N, H, W = a.shape
M = N * H * W
g = torch.Generator().manual_seed(0)
out = {"shape": [N, H, W], "rounds": a.rounds, "launches_per_round": a.reps * a.replays, "call_us": {}}


def rows(named):
    """Time the named calls (name -> (fn, bytes)) alternating inside every round."""
    ts = timing.time_calls({n: fn for n, (fn, _) in named.items()}, a.rounds, a.reps, a.replays)
    for n, (_, nbytes) in named.items():
        s = timing.spread(ts[n])
        out["call_us"][n] = dict(s, MB=round(nbytes / 1e6, 2), TBps=round(nbytes / s["median"] / 1e6, 3))
        print(f"  {n:52s} {s['median']:9.2f} us median ({s['min']:.2f} - {s['max']:.2f})   {nbytes / 1e6:7.2f} MB -> {nbytes / s['median'] / 1e6:5.2f} TB/s",
              flush=True)


# a sector scan's tables, and a bleed-like stack: discs and speckle as the prediction, the discs alone as the truth
r = 20.0 + 0.25 * np.arange(H)[:, None]
th = -0.5 + (1.0 / W) * np.arange(W)[None, :]
geo = ScanGeometry(r * np.sin(th), r * np.cos(th))
wq, xq, yq = geo.tables("cuda")
yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
cy, cx = torch.randint(10, H - 10, (N, 2, 1, 1), generator=g), torch.randint(10, W - 10, (N, 2, 1, 1), generator=g)
rad = torch.randint(3, 12, (N, 2, 1, 1), generator=g)
rad[1::2, 1] = 0                                                                 # every second image has one disc only
discs = (((yy - cy) ** 2 + (xx - cx) ** 2) < rad ** 2).any(1)
truth = discs.to(torch.uint8).cuda()
pred = (discs.roll((1, -1), (1, 2)) | (torch.rand((N, H, W), generator=g) < 0.01)).to(torch.uint8).cuda()
truth4 = (truth + 2 * (torch.rand((N, H, W), generator=g) < 0.3).to(torch.uint8).cuda()).contiguous()
pred4 = (pred + 2 * (torch.rand((N, H, W), generator=g) < 0.3).to(torch.uint8).cuda()).contiguous()


def check_confusion(p, q, C_, weight):
    cm, wcm, inv = ops.image_confusion(p, q, C_, weight)
    cell = (q.long() * C_ + p.long()).reshape(N, -1)
    want = torch.stack([(cell == c).sum(1) for c in range(C_ * C_)], 1).reshape(N, C_, C_)
    assert torch.equal(cm, want) and not inv.any()
    if weight is not None:
        wl = weight.long().reshape(1, -1)
        assert torch.equal(wcm, torch.stack([((cell == c) * wl).sum(1) for c in range(C_ * C_)], 1).reshape(N, C_, C_))


check_confusion(pred, truth, 2, None)
check_confusion(pred, truth, 2, wq)
check_confusion(pred4, truth4, 4, wq)
print(f"the calls at {N} x {H} x {W} ({M} pixels), {a.rounds} rounds of {a.replays} replays of {a.reps} calls, alternating:")
o2 = tuple(torch.empty(s, dtype=torch.int64, device="cuda") for s in ((N, 2, 2), (N, 2, 2), (N,)))
o4 = tuple(torch.empty(s, dtype=torch.int64, device="cuda") for s in ((N, 4, 4), (N, 4, 4), (N,)))
rows({"image_confusion C=2": (lambda: ops.image_confusion(pred, truth, 2, None, out=(o2[0], None, o2[2])), 2 * M),
      "image_confusion C=2, area weights": (lambda: ops.image_confusion(pred, truth, 2, wq, out=o2), 2 * M + 4 * H * W),
      "image_confusion C=4, area weights": (lambda: ops.image_confusion(pred4, truth4, 4, wq, out=o4), 2 * M + 4 * H * W)})

labels, count = ops.label_components(pred, 8)
cap = int(count.max())
out["components"] = {"total": int(count.sum()), "cap": cap}
table = ops.component_measure(labels, wq, xq, yq, cap)
onehot_px = torch.zeros(N * (cap + 1), dtype=torch.int64, device="cuda")
onehot_w = torch.zeros_like(onehot_px)
flat = (labels.long() + (cap + 1) * torch.arange(N, device="cuda").reshape(N, 1, 1)).reshape(-1)
onehot_px.index_add_(0, flat, torch.ones_like(flat))
onehot_w.index_add_(0, flat, wq.long().expand(N, H, W).reshape(-1))
assert torch.equal(table[..., 0], onehot_px.reshape(N, cap + 1)[:, 1:]) and torch.equal(table[..., 1], onehot_w.reshape(N, cap + 1)[:, 1:])
print(f"  ({int(count.sum())} components, at most {cap} in an image)")
rows({f"component_measure cap={cap}": (lambda: ops.component_measure(labels, wq, xq, yq, cap, out=table), 4 * M + 12 * H * W)})

K = 8
units = torch.randint(0, 1 << 30, (N, K), generator=g, dtype=torch.int64).cuda()
patients = units[:64].contiguous()
ops.bootstrap_check_rows(1 << 30, N)
first = ops.bootstrap_sums(units, 4, 1, check=False)
assert int(first.min()) > 0 and torch.equal(first, ops.bootstrap_sums(units, 1000, 1, check=False)[:4])
b1, b2 = torch.empty((1000, K), dtype=torch.int64, device="cuda"), torch.empty((10000, K), dtype=torch.int64, device="cuda")
rows({f"bootstrap_sums U={N} K=8 R=1000": (lambda: ops.bootstrap_sums(units, 1000, 1, out=b1, check=False), 8 * K * (N + 1000)),
      f"bootstrap_sums U={N} K=8 R=10000": (lambda: ops.bootstrap_sums(units, 10000, 1, out=b2, check=False), 8 * K * (N + 10000)),
      "bootstrap_sums U=64 K=8 R=10000": (lambda: ops.bootstrap_sums(patients, 10000, 1, out=b2, check=False), 8 * K * (64 + 10000))})
timing.write_json(a.json, out)
print("wrote", a.json)
