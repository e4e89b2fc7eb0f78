"""GPU half of MainParallel.py's epoch driver (tests/test_cpu_mainparallel.py is the host half).

  * Two ranks against a simulation: ``main`` in a world of two over gloo on device 0 (``torch.distributed.run`` as a child), 64x64x10,
    global batch 4, 9 training and 5 test images, so rank 1 holds nothing of either last batch; two epochs with the captured step.  The
    parent replays the same epochs eagerly with two model instances in one process: each computes its slice's clipped gradient, the two
    are summed, each applies the update.  Weights, Adam m / v / step, BatchNorm statistics, the reduced counters (through the metrics)
    and the losses agree bit for bit: a SUM of two addends is exact and order-free, and a step replayed from the graph is bitwise the
    eager step.  Both ranks end with bit-equal weights.
  * World 1: the driver with the graph equals the driver without it, over an epoch that ends in a 1-image batch.
  * ``train_step`` after ``capture_graph`` with a batch of another shape runs eagerly and equals a fresh eager model.
  * ``main`` at 256x80x10 with the ViT on a tiny ``.npy`` pair: the model rank 0 saves loads back into a fresh model."""
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
H, W, C = 64, 64, 10
B, N_TRAIN, N_TEST, EPOCHS, SEED = 4, 9, 5, 2, 11


def _arrays(n, h=H, w=W, seed=0):
    """The on-disk layout [N,1,H,W,12]: label (0 outside the brain, soft classes 0..2 inside), 10 displacement channels, bMode."""
    rng = np.random.default_rng(seed)
    a = np.empty((n, 1, h, w, 12), dtype=np.float64)
    lab = rng.random((n, h, w)) * 2.2
    lab[rng.random((n, h, w)) < 0.4] = 0.0
    a[:, 0, :, :, 0] = lab
    a[:, 0, :, :, 1:] = rng.standard_normal((n, h, w, 11)) * 0.3
    return a


def _state(net):
    """Everything a training step writes: flat weights, Adam moments and step counter, BatchNorm moving statistics."""
    torch.cuda.synchronize()
    d = {"flat": net.flat.flat.cpu(), "m": net.optimizer.m.cpu(), "v": net.optimizer.v.cpu(), "step": net.optimizer.step_dev.cpu()}
    d.update({k: v.cpu() for k, v in net.export_params().items() if k.endswith((".moving_mean", ".moving_variance"))})
    return d


def _first_difference(a, b):
    for k in a:
        if not torch.equal(a[k], b[k]):
            return k
    return None


def _same_history(h1, h2):
    assert len(h1) == len(h2)
    for a, b in zip(h1, h2):
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (a, b)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------- two ranks against a simulation
def _simulate(train, val):
    """The two replicas of ``main(epochs=EPOCHS, batch_size=B, use_vit=False, seed=SEED)`` in one process, eagerly."""
    from ultrasound_modeling_amd.Dataset import Dataset
    from ultrasound_modeling_amd.metrics import SegMetrics, counts_to_metrics
    from ultrasound_modeling_amd.step import _LocalSync
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    ds = Dataset(train_data=train, val_data=val, batch_size=B, device=DEV)
    nets = [VisionTransformer(B, img_size=(H, W), in_channels=C, device=DEV) for _ in range(2)]
    for n in nets:
        n.grad_sync = _LocalSync()            # the data-parallel order: per-replica clip in _grad_body, no clip inside Adam
    zero = torch.zeros((), dtype=torch.float32, device=DEV)
    rngs = [random.Random(SEED), random.Random(SEED)]
    history, it = [], 0
    for epoch in range(EPOCHS):
        mets = [SegMetrics(3, round=True, device=DEV) for _ in range(2)]
        last = [zero, zero]
        for pair in zip(ds.train_batches(0, 2, rngs[0]), ds.train_batches(1, 2, rngs[1])):
            for r, (x, y, _) in enumerate(pair):
                if x is None:
                    nets[r]._zero_grad()
                    last[r] = zero
                    continue
                probs = nets[r]._grad_body(x, y)
                last[r] = nets[r]._loss[0].clone()
                mets[r].update_state(y, probs)
            g = nets[0].flat.grad + nets[1].flat.grad
            for n in nets:
                n.flat.grad.copy_(g)
                n._update_body()
            it += 1
        m = counts_to_metrics(mets[0].counts + mets[1].counts)
        history.append(dict(m, phase="train", epoch=epoch, iteration=it, loss=float(last[0] + last[1])))
        mets = [SegMetrics(3, round=True, device=DEV) for _ in range(2)]
        totals = [zero.clone(), zero.clone()]
        for pair in zip(ds.test_batches(0, 2), ds.test_batches(1, 2)):
            for r, (x, y, _) in enumerate(pair):
                if x is not None:
                    loss, probs = nets[r].step(x, y)
                    totals[r].add_(loss.reshape(()))
                    mets[r].update_state(y, probs)
        m = counts_to_metrics(mets[0].counts + mets[1].counts)
        history.append(dict(m, phase="test", epoch=epoch, loss=float(totals[0] + totals[1])))
    return [_state(n) for n in nets], history


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
def test_two_ranks_equal_the_simulation_bit_for_bit(tmp_path):
    train, val = _arrays(N_TRAIN, seed=1), _arrays(N_TEST, seed=2)
    np.save(tmp_path / "train.npy", train)
    np.save(tmp_path / "val.npy", val)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "USSEG_DP_CHUNKS")}
    env.update(USSEG_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc_per_node", "2", "--master_addr", "127.0.0.1",
                        "--master_port", str(_free_port()), os.path.abspath(__file__), str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = [torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2)]
    assert d[0]["graph"] and d[1]["graph"]                                            # full local batches replayed the captured step
    assert torch.equal(d[0]["state"]["flat"], d[1]["state"]["flat"]), "replicas diverged"
    want, history = _simulate(train, val)
    for k in range(2):
        assert _first_difference(d[k]["state"], want[k]) is None, (k, _first_difference(d[k]["state"], want[k]))
    assert want[0]["step"].item() == EPOCHS * 3
    assert any(n.endswith(".moving_mean") for n in want[0])                            # the BatchNorm statistics were compared too
    _same_history(d[0]["history"], history)
    _same_history(d[1]["history"], history)


# ---------------------------------------------------------------------------------------------------- world 1
def _run_world1(capture, train, val):
    from ultrasound_modeling_amd.Dataset import Dataset
    from ultrasound_modeling_amd.MainParallel import Process
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    ds = Dataset(train_data=train, val_data=val, batch_size=B, device=DEV)
    net = VisionTransformer(B, img_size=(H, W), in_channels=C, device=DEV)
    proc = Process(B, capture_graph=capture)
    random.seed(SEED)
    proc.training(net, ds, 1, B)
    return net, proc


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
def test_world1_graph_equals_eager_with_a_one_image_last_batch():
    train, val = _arrays(N_TRAIN, seed=3), _arrays(N_TEST, seed=4)                    # 9 = 4 + 4 + 1
    g, pg = _run_world1(True, train, val)
    e, pe = _run_world1(False, train, val)
    assert g._graph is not None and e._graph is None
    sg, se = _state(g), _state(e)
    assert _first_difference(sg, se) is None, _first_difference(sg, se)
    assert sg["step"].item() == 3
    _same_history(pg.history, pe.history)
    assert [h["phase"] for h in pg.history] == ["train", "test"]


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
def test_mismatched_shape_after_capture_runs_eagerly():
    from ultrasound_modeling_amd.Dataset import Dataset
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    ds = Dataset(train_data=_arrays(3, seed=5), val_data=_arrays(1, seed=6), batch_size=2, device=DEV)
    params = [Dataset.draw(random.Random(7)) for _ in range(3)]
    x2, y2 = ds._augment(ds.x_tr[:2], ds.y_tr[:2], params[:2])
    x1, y1 = ds._augment(ds.x_tr[2:], ds.y_tr[2:], params[2:])
    cap = VisionTransformer(2, img_size=(H, W), in_channels=C, device=DEV)
    ref = VisionTransformer(2, img_size=(H, W), in_channels=C, device=DEV)
    cap.capture_graph(x2, y2)
    for x, y in ((x1, y1), (x2, y2), (x1, y1)):                                        # 1 image (eager), 2 (replay), 1 again
        lc, pc = cap.train_step(x, y)
        lr, pr = ref.train_step(x, y)
        torch.cuda.synchronize()
        assert pc.shape[0] == x.shape[0]
        assert torch.equal(lc.cpu(), lr.cpu()) and torch.equal(pc.cpu(), pr.cpu())
        assert _first_difference(_state(cap), _state(ref)) is None


# ---------------------------------------------------------------------------------------------------- main at the native shape
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")
def test_main_native_shape_saves_a_loadable_model(tmp_path):
    from ultrasound_modeling_amd.MainParallel import main
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    np.save(tmp_path / "train.npy", _arrays(3, 256, 80, seed=8))
    np.save(tmp_path / "val.npy", _arrays(2, 256, 80, seed=9))
    save = tmp_path / "model.pt"
    net, proc = main(str(tmp_path / "train.npy"), str(tmp_path / "val.npy"), str(save), epochs=1, batch_size=2, use_vit=True)
    assert net.transformer.encoder is not None and net.img_size == (256, 80)
    assert [h["phase"] for h in proc.history] == ["train", "test"] and np.isfinite(proc.history[0]["loss"])
    fresh = VisionTransformer(2, img_size=(256, 80), use_vit=True, device=DEV, seed=123)
    before = _state(fresh)
    fresh.load(str(save))
    a, b = _state(net), _state(fresh)
    assert _first_difference(a, b) is None, _first_difference(a, b)
    assert _first_difference(before, b) is not None
    assert a["step"].item() == 2


# ---------------------------------------------------------------------------------------------------- the rank process
def _rank(tmp):
    import torch.distributed as dist
    from ultrasound_modeling_amd.MainParallel import main
    net, proc = main(os.path.join(tmp, "train.npy"), os.path.join(tmp, "val.npy"), None, epochs=EPOCHS, batch_size=B, use_vit=False,
                     seed=SEED)
    rank = dist.get_rank()
    torch.save({"state": _state(net), "history": proc.history, "graph": net._graph is not None}, os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _rank(sys.argv[1])
