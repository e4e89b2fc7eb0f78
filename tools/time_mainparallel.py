"""Time per training step of MainParallel's epoch driver against the captured step alone.

    python tools/time_mainparallel.py [--batch-size 64] [--batches 8] [--epochs 3] [--no-vit]
    python -m torch.distributed.run --nproc_per_node 2 tools/time_mainparallel.py ...      (RCCL, one GPU per rank)

Driver: ``Process.mirrored_train_step`` over an epoch of full global batches of synthetic 256x80x10 samples (augment, captured DP step,
counter update per step; one loss / counter reduction at the end), the first epoch a warm-up that captures the graph; the time of each
later epoch / steps, max over ranks.  Captured step alone: ``train_step`` replays on one resident batch, same count.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8, help="global batches per epoch")
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs after the warm-up one")
    ap.add_argument("--no-vit", action="store_true")
    a = ap.parse_args()
    import torch.distributed as dist
    from ultrasound_modeling_amd.Dataset import Dataset
    from ultrasound_modeling_amd.MainParallel import Process, init_distributed
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    rank, world, local = init_distributed()
    dev = torch.device("cuda", local if world > 1 and dist.get_backend() == "nccl" else 0)
    torch.cuda.set_device(dev)
    n = a.batch_size * a.batches
    rng = np.random.default_rng(0)
    raw = np.empty((n, 1, 256, 80, 12), dtype=np.float64)
    lab = rng.random((n, 256, 80)) * 2.2
    lab[rng.random((n, 256, 80)) < 0.4] = 0.0
    raw[:, 0, :, :, 0] = lab
    raw[:, 0, :, :, 1:] = rng.standard_normal((n, 256, 80, 11)) * 0.3
    ds = Dataset(train_data=raw, val_data=raw[:a.batch_size], batch_size=a.batch_size, device=dev)
    del raw, lab
    net = VisionTransformer(a.batch_size, use_vit=not a.no_vit, device=str(dev))
    proc = Process(a.batch_size)
    proc._print = lambda *args, **kw: None
    proc.mirrored_train_step(net, ds)                                       # warm-up epoch: captures the step on its first batch
    per_epoch = []
    for _ in range(a.epochs):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        proc.mirrored_train_step(net, ds)                                   # ends in a host read of the reduced loss
        torch.cuda.synchronize()
        per_epoch.append(time.perf_counter() - t0)
    driver = min(per_epoch) / a.batches
    x, y = next(iter(ds.train_batches(proc.trainer.rank, proc.trainer.world)))[:2]
    step_times = []
    for _ in range(a.epochs):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            net.train_step(x, y)
        torch.cuda.synchronize()
        step_times.append(time.perf_counter() - t0)
    alone = min(step_times) / a.batches
    t = torch.tensor([driver, alone], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        d, s = t.tolist()
        print(json.dumps({"world": world, "global_batch": a.batch_size, "vit": not a.no_vit, "steps_per_epoch": a.batches,
                          "driver_ms_per_step": round(d * 1e3, 3), "captured_step_ms": round(s * 1e3, 3),
                          "overhead_pct": round(100.0 * (d / s - 1.0), 2)}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
