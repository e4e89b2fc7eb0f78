"""GPU half of TBI_TransUNet.py's own script: ``usseg_augment`` with ``do_flip`` against the NumPy restatement of the script's
``dataAug`` (tests/test_cpu_transunet_script.py), bit for bit in fp32 with the bf16 output the rounding of the fp32 one; the flip-off
path byte-identical to ``DataAugs``; the script's ``Dataset``; and ``training`` / ``test`` end to end at 256x80x10, batch 16
(determinism, the test F1 recomputed on the host, a captured train step)."""
import math
import random

import numpy as np
import pytest
import torch

import input_oracle as IO
from test_cpu_metrics import assert_metrics_equal, keras_metrics
from test_cpu_transunet_script import script_data_aug

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _data(seed, B=4, H=256, W=80, Cc=10):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, Cc)) * 0.3
    lab = rng.random((B, H, W)).astype(np.float32) * 2.2
    lab[rng.random((B, H, W)) < 0.4] = 0.0                                    # outside-the-brain pixels: label exactly 0
    lab[:, :, : W // 3][rng.random((B, H, W // 3)) < 0.4] = 0.0               # left-right asymmetric, so a missing flip shows
    return x, lab


def _check(x, lab, params, seed):
    """Kernel (fp64 input, injected noise) against the restatement: fp32 x, label and y_vec exact; bf16 x the rounding of fp32 x."""
    from ultrasound_modeling_amd import TBI_TransUNet as T
    gauss = np.random.default_rng(seed + 50).standard_normal(x.shape).astype(np.float32)
    ref_x, ref_y = np.zeros_like(x), np.zeros_like(lab)
    for b in range(x.shape[0]):
        ref_x[b], ref_y[b] = script_data_aug(x[b], lab[b], params[b], gauss[b].astype(np.float64))
    xo, yv, xf, ya = T.dataAug_batch(torch.tensor(x).to(DEV), torch.tensor(lab).to(DEV), params=params, noise=torch.tensor(gauss).to(DEV),
                                     want_f32=True)
    torch.cuda.synchronize()
    Cc = x.shape[-1]
    np.testing.assert_array_equal(ya.cpu().numpy(), ref_y.astype(np.float32))
    np.testing.assert_array_equal(xf.cpu().numpy(), ref_x.astype(np.float32))
    np.testing.assert_array_equal(yv.cpu().numpy(), IO.label2vec(ref_y.astype(np.float32), 3).astype(np.float32))
    assert (xo[..., Cc:] == 0).all()
    assert torch.equal(xo[..., :Cc].cpu(), torch.tensor(ref_x.astype(np.float32)).to(torch.bfloat16))
    return ref_x, ref_y


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 7])
def test_augment_matches_the_scripts_dataaug(seed):
    from ultrasound_modeling_amd import TBI_TransUNet as T
    x, lab = _data(seed)
    rng = random.Random(300 + seed)
    params = [T.draw(rng) for _ in range(x.shape[0])]
    _check(x, lab, params, seed)


def _forced(flip):
    base = dict(flip=flip, reduc=False, reduc_t=0, clips=[], shift=None, noise=False, seed=0)
    return [dict(base, reduc=True, reduc_t=3),
            dict(base, clips=[(40, 70, 30, 15)]),                            # a box at the right edge: its mirror is on the left
            dict(base, shift=(7, 5, 0)),
            dict(base, shift=(11, 9, 1)),
            dict(base, noise=True),
            dict(base, reduc=True, reduc_t=1, clips=[(200, 3, 25, 12)], shift=(3, 12, 1), noise=True)]


@pytest.mark.parametrize("flip", [False, True])
def test_augment_forced_parameters_cross_the_flip(flip):
    x, lab = _data(20, B=6)
    ref_x, _ = _check(x, lab, _forced(flip), 20)
    if flip:                                                                  # the flip is visible in each case
        ref_off, _ = _check(x, lab, _forced(False), 20)
        for b in range(6):
            assert not np.array_equal(ref_x[b], ref_off[b]), b


@pytest.mark.parametrize("seed", [0, 1])
def test_augment_odd_width(seed):
    from ultrasound_modeling_amd import TBI_TransUNet as T
    x, lab = _data(40 + seed, B=8, H=64, W=47, Cc=3)
    rng = random.Random(500 + seed)
    params = [T.draw(rng) for _ in range(2)] + _forced(True)
    params[0]["flip"], params[1]["flip"] = True, True
    params[2]["clips"] = [(30, 44, 20, 10)]
    params[3]["shift"] = (1, 1, 0)
    params[4]["shift"] = (1, 1, 1)
    _check(x, lab, params, 60 + seed)


def test_flip_off_is_dataaugs_byte_for_byte():
    from ultrasound_modeling_amd import DataAugs
    from ultrasound_modeling_amd import TBI_TransUNet as T
    x, lab = _data(30, B=6)
    xd, yd = torch.tensor(x).to(DEV), torch.tensor(lab).to(DEV)
    rng = random.Random(3)
    params = [dict(T.draw(rng), flip=False) for _ in range(6)]
    legacy = [{k: v for k, v in p.items() if k != "flip"} for p in params]   # DataAugs' draw format: no flip key
    a = T.dataAug_batch(xd, yd, params=params, want_f32=True)
    b = DataAugs.dataAug_batch(xd, yd, params=legacy, want_f32=True)        # noise from the per-sample generator in both
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.cpu().view(torch.uint8).numpy().tobytes() == v.cpu().view(torch.uint8).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------- Dataset
def _raw(n, h, w, seed):
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, 1, h, w, 12), dtype=np.float64)          # label, 10 displacement channels, bMode (TBI_TransUNet.py:643-655)
    raw[..., 1:11] = np.clip(rng.standard_normal((n, 1, h, w, 10)) * 0.3, -1, 1)
    raw[..., 0] = np.kron(rng.choice([0.0, 1.0, 1.3, 1.5, 2.0], size=(n, 1, h // 8, w // 8), p=[0.5, 0.2, 0.1, 0.1, 0.1]), np.ones((8, 8)))
    raw[..., 11] = 7.0                                          # bMode: must never reach the model
    return raw


def test_dataset_slices_terminators_and_model_input():
    from ultrasound_modeling_amd import TBI_TransUNet as T
    from ultrasound_modeling_amd import ops
    raw = _raw(5, 64, 64, seed=1)
    val = raw[:3]
    ds = T.Dataset(train_data=raw, val_data=val)
    assert (ds.num_tr, ds.num_te, ds.num_class, ds.channel) == (5, 3, 3, 10)
    B = 2
    for start, want_term, sl in ((0, False, slice(0, 2)), (2, False, slice(2, 4)), (4, True, slice(-3, -1)), (0, False, slice(0, 2))):
        assert ds.idx_tr == start
        random.seed(11 + start)
        x, y, term = ds.next_train(B)
        random.seed(11 + start)
        params = [T.draw() for _ in range(B)]
        xs = torch.tensor(raw[sl, 0, :, :, 1:-1]).to(DEV)
        ys = torch.tensor(raw[sl, 0, :, :, 0].astype(np.float32)).to(DEV)
        xw, yw = T.dataAug_batch(xs, ys, params=params)
        assert term == want_term and x.is_cuda and y.is_cuda and x.dtype == torch.bfloat16 and y.dtype == torch.float32
        assert x.shape == (B, 64, 64, 16) and y.shape == (B, 64, 64, 3)
        assert torch.equal(x, xw) and torch.equal(y, yw)
    x, y, term = ds.next_train(B, fix=True)                   # fix: the index stays
    assert ds.idx_tr == 2 and not term
    for want_term, sl in ((False, slice(0, 2)), (True, slice(-3, -1))):
        x, y, term = ds.next_test(B)
        assert term == want_term
        xs = torch.tensor(val[sl, 0, :, :, 1:-1]).to(DEV)
        assert torch.equal(x, ops.cast_input(xs.contiguous(), 16))
        assert torch.equal(y, T.label2vec(torch.tensor(val[sl, 0, :, :, 0].astype(np.float32)).to(DEV)))
    assert ds.idx_te == 0
    net = T.VisionTransformer(img_size=(64, 64), batch_size=B)
    x, y, _ = ds.next_train(B)
    loss, probs = net.step(x, y, train=True)
    loss_e, probs_e = net.step(*ds.next_test(B)[:2])
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and math.isfinite(float(loss_e)) and probs.shape == probs_e.shape == (B, 64, 64, 3)


# ---------------------------------------------------------------------------------------------------- training / test end to end
class _Recorder:
    """Delegates to the model and keeps (labels, probabilities) of every evaluation step."""

    def __init__(self, net):
        self.net, self.test = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def step(self, x, y, train=False):
        out = self.net.step(x, y, train=train)
        if not train:
            self.test.append((y.float().clone(), out[1].clone()))
        return out


@pytest.fixture(scope="module")
def script_run():
    from ultrasound_modeling_amd import TBI_TransUNet as T
    raw = _raw(60, 256, 80, seed=5)
    init = T.VisionTransformer().export_params()

    def run(graph=False):
        ds = T.Dataset(train_data=raw[:40], val_data=raw[40:])
        net = T.VisionTransformer()
        net.load_params(init)
        if graph:
            x0, y0, _ = ds.next_train(16)
            ds.reset_idx()
            net.capture_graph(x0, y0)
        rec = _Recorder(net)
        T.history.clear()
        random.seed(1234)
        steps = T.training(rec, ds, epochs=2, batch_size=16)
        torch.cuda.synchronize()
        return steps, [dict(h) for h in T.history], rec.test

    return run


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert set(u) == set(v)
        for k in u:
            assert (isinstance(u[k], float) and math.isnan(u[k]) and math.isnan(v[k])) or u[k] == v[k], (k, u[k], v[k])


def test_training_end_to_end_history_and_host_f1(script_run):
    steps, hist, tests = script_run()
    assert steps == 6                                          # 40 images, batch 16: 16, 16 and the short batch x[-17:-1]
    assert [(h["phase"], h["epoch"]) for h in hist] == [("train", 0), ("test", 0), ("train", 1)]
    assert all(math.isfinite(h["loss"]) for h in hist)
    assert [h["iteration"] for h in hist if h["phase"] == "train"] == [3, 6]
    assert len(tests) == 2                                     # 20 test images, batch 16: 16 and x[-17:-1]
    y = np.concatenate([t[0].cpu().numpy() for t in tests])
    p = np.concatenate([t[1].cpu().numpy() for t in tests])
    want = keras_metrics(y, p, rnd=True)
    assert_metrics_equal(hist[1], want)
    assert (math.isnan(want["f1"]) and math.isnan(hist[1]["f1"])) or hist[1]["f1"] == want["f1"]


def test_training_is_deterministic_and_the_graph_matches(script_run):
    _, first, _ = script_run()
    _, second, _ = script_run()
    _same(first, second)
    _, graphed, _ = script_run(graph=True)
    _same(graphed, first)
