"""Times the Lovasz-softmax loss (csrc/lovasz.hip) at the Arch B training shape, everything replayed from HIP graphs as tools/time_head.py does:

  * one training step of the model (``capture_graph``, then `rounds` rounds of `replays` replays between two events) for every ``--loss`` given -
    "lovasz_ce" against "dice_ce" is the comparison DESIGN.md section 8 quotes; ``--root DIR`` imports the package of ANOTHER checkout (the parent
    commit's, built there), so the baseline comes from the code that has no Lovasz loss at all: run the two trees alternately in one job;
  * with a library that has the loss: its launches at M = B*H*W pixels and C = 3 one group at a time - the coefficients call (16 launches), the
    sort alone (12 of them), the sums pass, the backward pass - each beside the bytes it must move.

usage: python tools/time_lovasz.py [--root DIR] [--loss NAME ...] [--rounds N] [--replays K] [--reps R] [--json PATH] [B H W]"""
import argparse
import os
import sys

import torch

import timing

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--loss", nargs="*", default=["dice_ce", "lovasz_ce", "lovasz"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--json", default=None)
ap.add_argument("shape", nargs="*", type=int, default=[16, 256, 80])
a = ap.parse_args()
B, H, W = a.shape
sys.path.insert(0, a.root)
from ultrasound_modeling_amd import _lib as L                                    # noqa: E402
from ultrasound_modeling_amd import ops                                         # noqa: E402
from ultrasound_modeling_amd.VisionTransformer import VisionTransformer         # noqa: E402

timing.require_gpu("time_lovasz")
out = {"root": a.root, "shape": [B, H, W], "step_ms": {}, "launch_us": {}}
g = torch.Generator().manual_seed(0)
x, y = timing.bleed_batch(B, H, W, 10, g)

print(f"{a.root}: Arch B {B} x {H} x {W} x 10, HIP-graph replay, {a.rounds} rounds of {a.replays} replays")
for name in a.loss:
    kw = {"overlap": {}} if name in ("dice", "tversky", "dice_ce") else {}
    net = VisionTransformer(batch_size=B, img_size=(H, W), loss=name, **kw)
    net.capture_graph(x, y)
    last = {}
    sp = timing.spread(timing.time_steps(lambda: last.update(loss=net.train_step(x, y)[0]), a.rounds, a.replays))
    l = float(last["loss"].item())
    out["step_ms"][name] = dict(sp, loss=l)
    print(f"  step, loss={name:10s} {sp['min']:8.4f} ms min, {sp['median']:8.4f} median, {sp['max']:8.4f} max   (loss {l:.5f})", flush=True)
    del net

if hasattr(L.load(), "usseg_lovasz_coeffs"):
    C_, M = 3, B * H * W
    probs = torch.softmax(2 * torch.randn(B, H, W, C_, generator=g), -1).cuda()
    gco, counts = torch.empty_like(probs), torch.zeros(4, dtype=torch.int32).cuda()
    ws = torch.empty(ops.lovasz_ws_bytes(M, C_), dtype=torch.uint8).cuda()
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS).cuda()
    dl = torch.empty(B, H // 2, W // 2, 16, dtype=torch.bfloat16).cuda()
    keys = torch.randint(0, 1 << 30, (C_, M), dtype=torch.int32).cuda()
    vals = torch.arange(C_ * M, dtype=torch.int32).reshape(C_, M).cuda()
    sws = torch.empty(ops.sort_ws_bytes(C_, M), dtype=torch.uint8).cuda()
    ll = ops.lovasz_loss([1.0] * C_, 1.0, 1.0)
    kw = dict(lovasz=ll, HW=H * W, C_classes=C_)
    n = C_ * M
    hist = C_ * ((M + ops.SORT_TILE - 1) // ops.SORT_TILE) * 256 * 4
    per_pass = 4 * n + 2 * hist + (8 * n + hist) + 8 * n                         # histogram read; offsets read + written; scatter: pairs read, offsets read, pairs written
    sort_b = 4 * per_pass
    print(f"the loss's launches at M = {M}, C = {C_} ({n} pairs), the calls alternating:")
    named = {"sort_pairs, 30 key bits": (lambda: ops.sort_pairs(keys, vals, 30, sws), 12, sort_b),
             "lovasz_coeffs (keys, sort, scan)": (lambda: ops.lovasz_coeffs(probs, y, gco, counts, ws, **kw), 16, 8 * n + 8 * n + sort_b + 4 * n + 4 * n + 4 * n),
             "lovasz_loss_sums": (lambda: ops.lovasz_loss_sums(probs, y, gco, counts, acc, inv_global_batch=1.0 / B, **kw), 1, 12 * n),
             "lovasz_loss_bwd (quad)": (lambda: ops.lovasz_loss_bwd(probs, y, gco, acc, dl, inv_global_batch=1.0 / B, quad_w=W, **kw), 1, 12 * n + 8 * M)}
    ts = timing.time_calls({k: fn for k, (fn, _, _) in named.items()}, a.rounds, a.reps, replays=3)
    for name, (_, launches, nbytes) in named.items():
        s = timing.spread(ts[name])
        out["launch_us"][name] = dict(s, launches=launches, MB=round(nbytes / 1e6, 1))
        print(f"  {name:34s} {launches:3d} launches {s['min']:8.2f} us min, {s['median']:8.2f} median, {s['max']:8.2f} max   {nbytes / 1e6:6.1f} MB -> "
              f"{nbytes / s['median'] / 1e6:5.2f} TB/s", flush=True)

if a.json:
    timing.write_json(a.json, out)
