"""Times knowledge distillation (csrc/distill.hip, ultrasound_modeling_amd/distill.py) at the benchmark's Arch B shape, everything replayed from HIP
graphs as tools/time_topk.py does:

  * the ONE launch of ``ops.distill_loss`` at M = B*H*W pixels, C = 3, quad layout, beside the bytes it must move - and, in the same run, its
    yardstick: the ``overlap_loss_sums`` + ``overlap_loss_bwd`` pair of "dice_ce" at the same shape (the pair reads p and y twice);
  * one training step of the model (``capture_graph``, then `replays` replays between two events) with ``loss="distill"`` and a one-member
    teacher, with a two-member ``Ensemble`` teacher, and with ``loss="cce"`` from THIS tree and - with ``--parent DIR``, a checkout of the parent
    commit built there - ``"cce"`` from the code that has no distillation at all.  The two trees run ALTERNATELY, one fresh process per tree and
    round, in one job on one box; the medians over the rounds are reported.

usage: python tools/time_distill.py [--parent DIR] [--rounds N] [--replays K] [--reps R] [--json PATH] [B H W]
       python tools/time_distill.py --child ROOT --case NAME ... [--replays K] [B H W]      (one round of one tree: prints a JSON line)"""
import argparse
import os
import sys

import timing

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--child", default=None)
ap.add_argument("--case", nargs="*", default=["cce", "distill1", "distill2"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--json", default=None)
ap.add_argument("shape", nargs="*", type=int, default=[16, 256, 256])
a = ap.parse_args()
B, H, W = a.shape


def child(root, cases):
    """One round of one tree: a captured Arch B step per case -> {case: ms per step}."""
    sys.path.insert(0, root)
    import torch
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    x, y = timing.bleed_batch(B, H, W, 1, torch.Generator().manual_seed(0))
    res = {}
    for name in cases:
        kw = {}
        if name.startswith("distill"):
            from ultrasound_modeling_amd.ensemble import Ensemble
            members = [VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1, seed=10 + i) for i in range(int(name[len("distill"):]))]
            kw = dict(loss="distill", teacher=members[0] if len(members) == 1 else Ensemble(members))
        net = VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1, **kw)
        net.capture_graph(x, y)
        res[name] = timing.time_steps(lambda: net.train_step(x, y), 1, a.replays)[0]
        del net
    timing.emit("TIME_DISTILL", res)


if a.child is not None:
    child(a.child, a.case)
    sys.exit(0)

import torch                                                                      # noqa: E402
sys.path.insert(0, HERE)
from ultrasound_modeling_amd import ops                                           # noqa: E402

timing.require_gpu("time_distill")
out = {"shape": [B, H, W], "launch_us": {}, "step_ms": {}}
C_, M = 3, B * H * W
g = torch.Generator().manual_seed(0)
probs = torch.softmax(2 * torch.randn(B, H, W, C_, generator=g), -1).cuda()
q = torch.softmax(3 * torch.randn(B, H, W, C_, generator=g), -1).cuda()
y = torch.nn.functional.one_hot(torch.randint(0, C_, (B, H, W), generator=g), C_).float().cuda()
settings = torch.tensor([2.0, 0.5, 0.5, 0.0]).cuda()
acc = torch.zeros(ops.DISTILL_ACC_FLOATS).cuda()
ov_acc = torch.zeros(ops.OVERLAP_ACC_FLOATS).cuda()
dl = torch.empty(B, H // 2, W // 2, 16, dtype=torch.bfloat16).cuda()

print(f"the distillation launch at M = {M}, C = {C_}, quad layout (HIP-graph replay, {a.rounds} rounds, the calls alternating):")
kw = dict(HW=H * W, C_classes=C_, inv_global_batch=1.0 / B)
ol = ops.overlap_loss([1.0 / C_] * C_, ce_weight=1.0)
named = {"distill_loss (p, y, q -> sums, dlogits)": (lambda: ops.distill_loss(probs, y, q, settings, acc, dl, quad_w=W, **kw), 1, 3 * 12 * M + 8 * M),
         "distill_loss, the loss alone": (lambda: ops.distill_loss(probs, y, q, settings, acc, None, quad_w=W, **kw), 1, 3 * 12 * M),
         "overlap_loss_sums + overlap_loss_bwd (dice_ce)": (lambda: (ops.overlap_loss_sums(probs, y, ov_acc, overlap=ol, ov_scale=1.0, **kw),
                                                                     ops.overlap_loss_bwd(probs, y, ov_acc, dl, overlap=ol, quad_w=W, **kw)), 2, 2 * 24 * M + 8 * M)}
ts = timing.time_calls({n: fn for n, (fn, _, _) in named.items()}, a.rounds, a.reps, replays=3)
for name, (_, launches, nbytes) in named.items():
    sp = timing.spread(ts[name], 2)
    out["launch_us"][name] = dict(sp, launches=launches, MB=round(nbytes / 1e6, 1))
    print(f"  {name:44s} {launches:2d} launches {sp['min']:8.2f} us min, {sp['median']:8.2f} median, {sp['max']:8.2f} max   {nbytes / 1e6:6.1f} MB -> "
          f"{nbytes / sp['median'] / 1e6:5.2f} TB/s", flush=True)
lu = out["launch_us"]
out["launch_vs_overlap_pair"] = round(lu["distill_loss (p, y, q -> sums, dlogits)"]["median"] / lu["overlap_loss_sums + overlap_loss_bwd (dice_ce)"]["median"], 3)
print(f"  distill_loss / the overlap pair: {out['launch_vs_overlap_pair']}")

trees = [("this", HERE, ["--case", *a.case])] + ([("parent", os.path.abspath(a.parent), ["--case", "cce"])] if a.parent else [])
print(f"Arch B {B} x {H} x {W} x 1 training step, HIP-graph replay, {a.rounds} rounds of {a.replays} replays, the trees alternating:")
runs = timing.alternate_trees(os.path.abspath(__file__), trees, a.rounds, "TIME_DISTILL", ["--replays", str(a.replays), str(B), str(H), str(W)], timeout=600)
for key, ts in runs.items():
    sp = timing.spread(ts)
    out["step_ms"][key] = dict(sp, rounds=[round(v, 4) for v in ts])
    print(f"  step, {key:18s} {sp['min']:8.4f} ms min, {sp['median']:8.4f} median, {sp['max']:8.4f} max", flush=True)
base = out["step_ms"].get("parent:cce", out["step_ms"].get("this:cce"))
if base:
    for key, v in out["step_ms"].items():
        v["vs_cce_us"] = round((v["median"] - base["median"]) * 1e3, 1)
if a.json:
    timing.write_json(a.json, out)
