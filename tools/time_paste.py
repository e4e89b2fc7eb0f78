"""Times the lesion copy-paste of one training batch inside captured HIP graphs, and shows that the default step does
not move:
  * ``usseg_lesion_paste`` at 16 x 256 x 80 x 10 fp64 against a synthetic bank of 64 records (one block lesion each, seeded), every sample
    active with the default settings; a ``clone()`` of the same ``x`` and ``y`` - the same bytes in and out with nothing decided; and, for
    scale, ``usseg_elastic_warp`` and ``usseg_augment`` on the same batch.  The four alternate inside every round (tools/timing.py).  The
    batch is 26 MB, so the launch ramp is a large share of each: the figure that means something is the ratio of the paste to the clone pair,
    printed with its min and max over the rounds;
  * with ``--parent DIR`` (a checkout of the parent commit, built there): ``bench.py --gpus 1 --steps 30 --warmup 10`` of the parent tree and
    of this tree, alternating, one fresh process per tree and round; the images/s of both, and whether the final loss is the same fp32 bits.

usage: python tools/time_paste.py [--parent DIR] [--rounds N] [--reps R] [--iters I] [--json PATH]
       python tools/time_paste.py --child ROOT [--steps K] [--warmup W]        (one benchmark run of one tree: prints a JSON line)"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

import timing

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (16, 256, 80, 10)
BANK = 64
SPREAD = 0.04                   # the box-to-box spread of the benchmark the README states


def child(root, steps, warmup):
    """One benchmark run of the tree at ``root`` in a process of its own -> the tagged line."""
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--no-cpu-baseline", "--dump-outputs", tmp], cwd=root, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit(f"bench.py of {root}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        loss = np.load(os.path.join(tmp, "loss.npy")).astype(np.float32).reshape(-1)
    timing.emit("TIME_PASTE", {"images_per_s": res["value"], "ms_per_step": res["ms_per_step"], "loss_bits": int(loss.view(np.int32)[0]),
                               "loss": float(loss[0])})


def kernels(a):
    import ctypes as C

    import torch

    sys.path.insert(0, HERE)
    from ultrasound_modeling_amd import DataAugs, _lib as L, ops, paste as Pp, warp as Wp
    B, H, W, Cc = SHAPE
    g = torch.Generator(device="cuda").manual_seed(1)
    x_bank = torch.randn((BANK, H, W, Cc), generator=g, device="cuda", dtype=torch.float64)
    y_bank = torch.ones((BANK, H, W), device="cuda")
    y_bank[:, 0, :] = 0
    y_bank[:, :, 0] = 0
    rng = random.Random(2)
    for n in range(BANK):                                       # one 12 x 10 lesion per record, inside the brain
        r, c = rng.randint(1, H - 13), rng.randint(1, W - 11)
        y_bank[n, r:r + 12, c:c + 10] = 2.0
    x, y = x_bank[:B].clone(), torch.ones((B, H, W), device="cuda")
    y[:, 0, :] = 0
    y[:, :, 0] = 0
    cfg = Pp.paste_config({"p": 1.0})
    bank = Pp.LesionBank(y_bank, cfg["connectivity"], cfg["min_area"])
    draws = [Pp.draw_paste(rng, cfg, bank, H, W) for _ in range(B)]
    table = Pp.sample_table(draws, x.device)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    landed = torch.empty((B, L.PASTE_MAX_ITEMS), dtype=torch.int32, device="cuda")
    xp, yp, xc, yc, xw, yw = (torch.empty_like(t) for t in (x, y, x, y, x, y))
    aug_table = DataAugs._sample_table([DataAugs.draw(rng) for _ in range(B)], x.device)
    wcfg = Wp.warp_config(dict(p=1.0))
    warp_table = Wp.sample_table([Wp.draw_warp(rng, wcfg, H, W) for _ in range(B)], x.device)
    weights = Wp.device_weights(wcfg["sigma"], x.device)
    cp = ops.roundup(Cc, 8)
    xo = torch.empty((B, H, W, cp), dtype=torch.bfloat16, device="cuda")
    yv = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
    lib, desc = L.load(), L.AugDesc(B, H, W, Cc, cp, 3)

    def paste():
        Pp.lesion_paste(x, y, table, x_bank, y_bank, bank.labels, protect=cfg["protect"], counts=counts, out=(xp, yp), landed=landed)

    def clone():
        xc.copy_(x)
        yc.copy_(y)

    def warp():
        Wp.elastic_warp(x, y, warp_table, weights, out=(xw, yw))

    def augment():
        L.check(lib.usseg_augment(C.byref(desc), aug_table.data_ptr(), x.data_ptr(), 1, y.data_ptr(), None, xo.data_ptr(), None, None, yv.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "augment")
    ts = timing.time_calls({"paste": paste, "clone": clone, "warp": warp, "augment": augment}, a.iters, a.reps, replays=1)
    counts.zero_()
    paste()
    torch.cuda.synchronize()
    placed, pixels = (int(v) for v in counts.cpu())
    ratios = [p / c for p, c in zip(ts["paste"], ts["clone"])]
    nbytes = 2 * B * H * W * (Cc * 8 + 4)
    out = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "dtype": "float64", "bank_records": BANK, "lesions_in_bank": len(bank),
           "lesions_drawn": sum(d["n"] for d in draws), "lesions_placed": placed, "pixels_pasted": pixels, "reps": a.reps, "iters": a.iters,
           "unit": "us per call; min / upper median / max over the rounds", "bytes_in_and_out": nbytes,
           "us": {k: timing.spread(v, 2) for k, v in ts.items()}, "paste_over_clone": timing.spread(ratios, 3)}
    for k, v in out["us"].items():
        print(f"  {k:8s} {v['min']:8.2f} us min, {v['median']:8.2f} median, {v['max']:8.2f} max", flush=True)
    r = out["paste_over_clone"]
    print(f"  paste / clone pair: {r['median']:.3f} (min {r['min']:.3f}, max {r['max']:.3f}); {placed} of {out['lesions_drawn']} lesions placed, "
          f"{pixels} pixels; {nbytes / 1e6:.1f} MB in and out", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--json", default=os.path.join(HERE, "profiles", "paste_step.json"))
    a = ap.parse_args()
    timing.require_gpu("time_paste")
    if a.child:
        return child(os.path.abspath(a.child), a.steps, a.warmup)
    out = {"kernel": kernels(a)}
    if a.parent:
        trees = [("parent", os.path.abspath(a.parent), []), ("this", HERE, [])]
        runs = timing.alternate_trees(os.path.abspath(__file__), trees, a.rounds, "TIME_PASTE", ["--steps", str(a.steps), "--warmup", str(a.warmup)], timeout=900)
        bits = {k: sorted(set(v)) for k, v in runs.items() if k.endswith(":loss_bits")}
        med = {k: timing.spread(runs[k + ":images_per_s"], 2) for k in ("parent", "this")}
        ratio = med["this"]["median"] / med["parent"]["median"]
        out["bench"] = {"command": f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup} --no-cpu-baseline --dump-outputs DIR", "rounds": a.rounds,
                        "images_per_s": {k: dict(med[k], rounds=runs[k + ":images_per_s"]) for k in med}, "this_over_parent": round(ratio, 4),
                        "inside_the_spread": abs(ratio - 1) <= SPREAD, "final_loss": {k.split(":")[0]: runs[k.split(":")[0] + ":loss"][0] for k in bits},
                        "final_loss_bit_equal": len(set(b for v in bits.values() for b in v)) == 1}
        b = out["bench"]
        print(f"  bench: parent {med['parent']['median']:.1f} images/s, this {med['this']['median']:.1f} ({ratio:.4f}x; inside +-{SPREAD:.0%}: {b['inside_the_spread']}); "
              f"final loss bit-equal: {b['final_loss_bit_equal']} ({b['final_loss']})", flush=True)
    else:
        out["bench"] = "not measured in this run (no --parent)"
    timing.write_json(a.json, out)


if __name__ == "__main__":
    main()
