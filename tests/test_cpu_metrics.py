"""CPU tests of the validation metrics (ultrasound_modeling_amd/metrics.py, include/usseg.h usseg_seg_counts): a NumPy restatement
of the Keras rules the reference's drivers score with (MainNumpy.py:49-53,97-147; TBI_ResNest.py:413-449), known answers for it,
``counts_to_metrics`` against it, the exact SUM reduction over two gloo ranks, and the C ABI's argument checks.  The GPU tests
(tests/test_gpu_metrics.py) hold the kernel to ``np_counts`` below, bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOUNTS = 23


# ---------------------------------------------------------------------------------------------------- the restatement
def _prepare(y_true, y_pred, rnd):
    y, p = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
    if rnd:                              # tf.math.round: half to even, as np.rint
        y, p = np.rint(y), np.rint(p)
    return y, p


def _pr_counts(y, p):
    """Keras Precision / Recall: y_true cast to bool, y_pred > 0.5 (the default threshold)."""
    t, q = y != 0, p > 0.5
    return int(np.sum(t & q)), int(np.sum(~t & q)), int(np.sum(t & ~q))


def _cm(y, p, nc):
    """tf.math.confusion_matrix on the flattened values cast to int64 (truncation), as MeanIoU calls it; None when TF would raise."""
    y, p = y.reshape(-1), p.reshape(-1)
    if not (np.all(y > -1) and np.all(y < nc) and np.all(p > -1) and np.all(p < nc)):
        return None
    cm = np.zeros((nc, nc), np.int64)
    np.add.at(cm, (np.trunc(y).astype(np.int64), np.trunc(p).astype(np.int64)), 1)
    return cm


def np_counts(y_true, y_pred, nc=3, rnd=True):
    """The USSEG_SEG_COUNTS int64 counters of a [B,H,W,C] batch, element by element as include/usseg.h states the rules."""
    y, p = _prepare(y_true, y_pred, rnd)
    out = np.zeros(NCOUNTS, np.int64)
    out[0:3] = _pr_counts(y, p)
    out[3:6] = _pr_counts(y[:, :, -1], p[:, :, -1])            # the reference's `c2`: the last image column
    t_ok = (y > -1) & (y < nc)
    p_ok = (p >= 0) & (p <= 1) & (p < nc)
    ok = t_ok & p_ok
    cm = np.zeros((nc, nc), np.int64)
    np.add.at(cm, (np.trunc(y[ok]).astype(np.int64), np.trunc(p[ok]).astype(np.int64)), 1)
    out[6:6 + nc * nc] = cm.reshape(-1)
    out[6 + nc * nc] = int(np.sum(~ok))
    return out


def keras_metrics(y_true, y_pred, nc=3, rnd=True):
    """What the driver reads from its Keras objects, computed from the tensors (not from counters); raises ValueError where TF raises."""
    y, p = _prepare(y_true, y_pred, rnd)
    if np.any(p < 0) or np.any(p > 1) or np.any(np.isnan(p)):
        raise ValueError("predictions must be in [0, 1]")
    cm = _cm(y, p, nc)
    if cm is None:
        raise ValueError("confusion_matrix: labels out of range")
    dnn = lambda a, b: a / b if b else 0.0
    f1 = lambda a, b: 2 * a * b / (a + b) if a + b else float("nan")
    tp, fp, fn = _pr_counts(y, p)
    tp2, fp2, fn2 = _pr_counts(y[:, :, -1], p[:, :, -1])
    P, R, P2, R2 = dnn(tp, tp + fp), dnn(tp, tp + fn), dnn(tp2, tp2 + fp2), dnn(tp2, tp2 + fn2)
    denom = cm.sum(0) + cm.sum(1) - np.diag(cm)
    valid = denom != 0
    miou = dnn(float(np.sum(np.diag(cm)[valid] / denom[valid])), int(valid.sum()))
    return {"precision": P, "recall": R, "f1": f1(P, R), "c2_precision": P2, "c2_recall": R2, "c2_f1": f1(P2, R2), "mean_iou": miou}


def assert_metrics_equal(a, b, tol=1e-12):
    assert set(a) >= set(b), (sorted(a), sorted(b))
    for k in b:
        if math.isnan(b[k]):
            assert math.isnan(a[k]), (k, a[k])
        else:
            assert abs(a[k] - b[k]) <= tol, (k, a[k], b[k])


def random_batch(shape, seed, nc=3):
    """Softmax probabilities with planted exact 0.5 values, and label2vec of labels that include exactly 1.5 (-> a label of 0.5)."""
    rng = np.random.default_rng(seed)
    B, H, W, Cc = shape
    z = rng.standard_normal(shape).astype(np.float32) * 2
    p = np.exp(z - z.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    flat = p.reshape(-1)
    flat[rng.choice(flat.size, max(1, flat.size // 50), replace=False)] = 0.5
    import input_oracle as IO
    if Cc == 3:      # 1.5 -> [0, 0.5, 0.5]
        lab = rng.choice(np.array([0, 0.5, 1, 1.5, 2], np.float32), size=(B, H, W))
        lab.reshape(-1)[rng.choice(lab.size, max(1, lab.size // 20), replace=False)] = 1.5
        y = IO.label2vec(lab, 3).astype(np.float32)
    elif Cc == 2:    # 0.5 -> [0.5, 0.5]
        lab = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], np.float32), size=(B, H, W))
        y = IO.label2vec(lab, 2).astype(np.float32)
    else:
        y = np.eye(Cc, dtype=np.float32)[rng.integers(0, Cc, size=(B, H, W))]
    return y, p


# ---------------------------------------------------------------------------------------------------- known answers
def _t(rows):
    return np.asarray(rows, np.float32)[None, None]        # [1,1,W,C]


def test_ties_at_one_half_round_to_even():
    y = _t([[0.5, 1.0, 0.0], [0.0, 0.5, 1.0]])
    p = _t([[0.5, 0.6, 0.4], [0.7, 0.5, 0.2]])
    # rounded: y -> [0,1,0],[0,0,1]  p -> [0,1,0],[1,0,0]  (0.5 -> 0 in both)
    c = np_counts(y, p)
    assert list(c[:6]) == [1, 1, 1, 0, 1, 1]
    cm = c[6:15].reshape(3, 3)
    assert cm.tolist() == [[3, 1, 0], [1, 1, 0], [0, 0, 0]] and c[15] == 0
    m = keras_metrics(y, p)
    assert m["precision"] == 0.5 and m["recall"] == 0.5 and m["f1"] == 0.5
    assert m["c2_precision"] == 0.0 and m["c2_recall"] == 0.0 and math.isnan(m["c2_f1"])
    # class 2 is absent from both tensors: left out of the mean (IoU0 = 3/5, IoU1 = 1/3)
    assert abs(m["mean_iou"] - (3 / 5 + 1 / 3) / 2) < 1e-12


def test_soft_labels_without_rounding():
    y, p = _t([[0.3, 0.7, 0.0]]), _t([[0.2, 0.9, 0.1]])
    m = keras_metrics(y, p, rnd=False)                     # 0.3 is a positive label unrounded (TBI_ResNest.py:423-426)
    assert m["precision"] == 1.0 and m["recall"] == 0.5 and abs(m["f1"] - 2 / 3) < 1e-12
    assert m["mean_iou"] == 1.0                            # every value truncates to class 0
    assert m["c2_recall"] == 0.5                           # W = 1: the last column is the whole image
    m = keras_metrics(y, p, rnd=True)
    assert m["precision"] == 1.0 and m["recall"] == 1.0


def test_no_predicted_positives():
    y = _t([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = np.full_like(y, 0.1)
    m = keras_metrics(y, p)
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and math.isnan(m["f1"])
    from ultrasound_modeling_amd.metrics import counts_to_metrics
    assert_metrics_equal(counts_to_metrics(torch.from_numpy(np_counts(y, p))), m)     # NaN, no ZeroDivisionError


@pytest.mark.parametrize("y_bad,p_bad", [(3.0, None), (-1.0, None), (None, 1.7), (None, -0.7), (None, float("nan"))])
def test_invalid_element_raises(y_bad, p_bad):
    from ultrasound_modeling_amd.metrics import counts_to_metrics
    y, p = _t([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]), _t([[0.2, 0.7, 0.1], [0.6, 0.3, 0.1]])
    if y_bad is not None:
        y[0, 0, 1, 2] = y_bad
    if p_bad is not None:
        p[0, 0, 1, 2] = p_bad
    for rnd in (True, False):                               # (values that round into range, like 1.2 or -0.1, are valid when rounded)
        with pytest.raises(ValueError):
            keras_metrics(y, p, rnd=rnd)
        c = np_counts(y, p, rnd=rnd)
        assert c[15] == 1
        with pytest.raises(ValueError):
            counts_to_metrics(torch.from_numpy(c))


# ---------------------------------------------------------------------------------------------------- counts_to_metrics
@pytest.mark.parametrize("shape,nc", [((2, 8, 5, 3), 3), ((3, 7, 5, 3), 3), ((2, 6, 4, 2), 2), ((2, 5, 1, 3), 3), ((1, 4, 4, 4), 4)])
@pytest.mark.parametrize("rnd", [True, False])
def test_counts_to_metrics_matches_restatement(shape, nc, rnd):
    from ultrasound_modeling_amd.metrics import counts_to_metrics
    y, p = random_batch(shape, seed=sum(shape) + nc, nc=nc)
    c = np_counts(y, p, nc, rnd)
    assert c[6 + nc * nc] == 0 and c[6:6 + nc * nc].sum() == y.size
    assert_metrics_equal(counts_to_metrics(torch.from_numpy(c), nc), keras_metrics(y, p, nc, rnd))


def test_metrics_object_has_no_cpu_update():
    from ultrasound_modeling_amd.metrics import SegMetrics
    m = SegMetrics(3, device="cpu")
    y, p = random_batch((1, 4, 4, 3), seed=1)
    with pytest.raises(RuntimeError):
        m.update_state(torch.from_numpy(y), torch.from_numpy(p))
    m.counts.copy_(torch.from_numpy(np_counts(y, p)))
    assert_metrics_equal(m.result(), keras_metrics(y, p))
    m.reset_states()
    assert int(m.counts.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------- two replicas
def _reduce_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    from ultrasound_modeling_amd.metrics import SegMetrics
    dist.init_process_group("gloo", rank=rank, world_size=world)
    y, p = random_batch((4, 9, 6, 3), seed=21)
    n = y.shape[0] // world
    m = SegMetrics(3, device="cpu")
    m.counts.copy_(torch.from_numpy(np_counts(y[rank * n:(rank + 1) * n], p[rank * n:(rank + 1) * n])))
    m.reduce()
    torch.save({"counts": m.counts.clone(), "metrics": m.result()}, os.path.join(tmp, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_world2_gloo_is_exact(tmp_path):
    """SegMetrics.reduce over two ranks' counters == the counters of the whole batch, exactly (replaces the reference's gather of
    probabilities and labels, MainParallel.py:148-176)."""
    from ultrasound_modeling_amd.metrics import counts_to_metrics
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_reduce_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    y, p = random_batch((4, 9, 6, 3), seed=21)
    whole = torch.from_numpy(np_counts(y, p))
    for r in range(2):
        got = torch.load(tmp_path / f"r{r}.pt")
        assert torch.equal(got["counts"], whole)
        assert got["metrics"] == counts_to_metrics(whole) or all(
            (math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(got["metrics"].values(), counts_to_metrics(whole).values()))


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_seg_counts_bad_arguments_without_touching_a_gpu():
    from ultrasound_modeling_amd import _lib
    lib = _lib.load()
    assert _lib.SEG_COUNTS == NCOUNTS
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    assert f"#define USSEG_SEG_COUNTS {NCOUNTS}" in hdr
    d = _lib.SegCountDesc(2, 4, 4, 3, 3, 1)
    assert lib.usseg_seg_counts(C.byref(d), 16, None, 16, None) == -1 and b"null pointer" in lib.usseg_last_error()
    assert lib.usseg_seg_counts(None, 16, 16, 16, None) == -1 and b"null pointer" in lib.usseg_last_error()
    for bad in (dict(num_classes=0), dict(num_classes=5), dict(round=2), dict(W=0), dict(C=0), dict(B=-1)):
        d = _lib.SegCountDesc(2, 4, 4, 3, 3, 1)
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib.usseg_seg_counts(C.byref(d), 16, 16, 16, None) == -1, bad
        assert b"bad descriptor" in lib.usseg_last_error(), bad
