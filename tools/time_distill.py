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
import json
import os
import subprocess
import sys

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


def median(ts):
    return sorted(ts)[len(ts) // 2]


def child(root, cases):
    """One round of one tree: a captured Arch B step per case -> {case: ms per step}."""
    sys.path.insert(0, root)
    import torch
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, H, W, 1, generator=g).clamp_(-1, 1).cuda()
    lab = torch.zeros(B, H, W, dtype=torch.long)
    lab[:, H // 3:H // 3 + H // 8, W // 3:W // 3 + W // 8] = 2                   # a bleed class of about 1.5 % of the pixels inside a band of class 1
    lab[:, H // 4:3 * H // 4, :][lab[:, H // 4:3 * H // 4, :] == 0] = 1
    y = torch.nn.functional.one_hot(lab, 3).float().cuda()
    res = {}
    for name in cases:
        kw = {}
        if name.startswith("distill"):
            from ultrasound_modeling_amd.ensemble import Ensemble
            members = [VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1, seed=10 + i) for i in range(int(name[len("distill"):]))]
            kw = dict(loss="distill", teacher=members[0] if len(members) == 1 else Ensemble(members))
        net = VisionTransformer(batch_size=B, img_size=(H, W), in_channels=1, **kw)
        net.capture_graph(x, y)
        for _ in range(5):
            net.train_step(x, y)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.replays):
            net.train_step(x, y)
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / a.replays
        del net
    print("TIME_DISTILL " + json.dumps(res), flush=True)


if a.child is not None:
    child(a.child, a.case)
    sys.exit(0)

import torch                                                                      # noqa: E402
sys.path.insert(0, HERE)
from ultrasound_modeling_amd import ops                                           # noqa: E402

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


def t(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(a.reps):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (3 * a.reps) * 1e3


def row(name, fn, launches, nbytes):
    ts = sorted(t(fn) for _ in range(a.rounds))
    out["launch_us"][name] = dict(min=round(ts[0], 2), median=round(median(ts), 2), max=round(ts[-1], 2), launches=launches, MB=round(nbytes / 1e6, 1))
    print(f"  {name:44s} {launches:2d} launches {ts[0]:8.2f} us min, {median(ts):8.2f} median, {ts[-1]:8.2f} max   {nbytes / 1e6:6.1f} MB -> "
          f"{nbytes / median(ts) / 1e6:5.2f} TB/s", flush=True)


print(f"the distillation launch at M = {M}, C = {C_}, quad layout (HIP-graph replay, {a.rounds} rounds):")
kw = dict(HW=H * W, C_classes=C_, inv_global_batch=1.0 / B)
ol = ops.overlap_loss([1.0 / C_] * C_, ce_weight=1.0)
row("distill_loss (p, y, q -> sums, dlogits)", lambda: ops.distill_loss(probs, y, q, settings, acc, dl, quad_w=W, **kw), 1, 3 * 12 * M + 8 * M)
row("distill_loss, the loss alone", lambda: ops.distill_loss(probs, y, q, settings, acc, None, quad_w=W, **kw), 1, 3 * 12 * M)
row("overlap_loss_sums + overlap_loss_bwd (dice_ce)", lambda: (ops.overlap_loss_sums(probs, y, ov_acc, overlap=ol, ov_scale=1.0, **kw),
                                                              ops.overlap_loss_bwd(probs, y, ov_acc, dl, overlap=ol, quad_w=W, **kw)), 2, 2 * 24 * M + 8 * M)
lu = out["launch_us"]
out["launch_vs_overlap_pair"] = round(lu["distill_loss (p, y, q -> sums, dlogits)"]["median"] / lu["overlap_loss_sums + overlap_loss_bwd (dice_ce)"]["median"], 3)
print(f"  distill_loss / the overlap pair: {out['launch_vs_overlap_pair']}")

trees = [("this", HERE, a.case)] + ([("parent", os.path.abspath(a.parent), ["cce"])] if a.parent else [])
runs = {}
print(f"Arch B {B} x {H} x {W} x 1 training step, HIP-graph replay, {a.rounds} rounds of {a.replays} replays, the trees alternating:")
for r in range(a.rounds):
    for tag, root, cases in trees:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--case", *cases, "--replays", str(a.replays), str(B), str(H), str(W)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"{tag} tree, round {r}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")        # nothing more is started after a failure
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("TIME_DISTILL ")][-1]
        for name, ms in json.loads(line[len("TIME_DISTILL "):]).items():
            runs.setdefault(f"{tag}:{name}", []).append(ms)
for key, ts in runs.items():
    out["step_ms"][key] = dict(min=round(min(ts), 4), median=round(median(ts), 4), max=round(max(ts), 4), rounds=[round(v, 4) for v in ts])
    print(f"  step, {key:18s} {min(ts):8.4f} ms min, {median(ts):8.4f} median, {max(ts):8.4f} max", flush=True)
base = out["step_ms"].get("parent:cce", out["step_ms"].get("this:cce"))
if base:
    for key, v in out["step_ms"].items():
        v["vs_cce_us"] = round((v["median"] - base["median"]) * 1e3, 1)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
