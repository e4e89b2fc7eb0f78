"""TBI_TransUNet.py's own script on the host side: the draws of its ``dataAug`` (:835-875) against a literal restatement of the
``random.randint`` calls, the NumPy restatement of that ``dataAug`` (flip first, imageReduc with an inert count, one clip box, shift,
noise) pinned against hand-built answers, the ``do_flip`` field of the C ABI, the Dataset's draw hook, and the control flow of
``training`` (test epochs, the fixed rate by default, the installed schedule) with stub model, data and metrics: no kernel runs.
The GPU half is tests/test_gpu_transunet_script.py."""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

import input_oracle as IO
from ultrasound_modeling_amd import TBI_TransUNet as T
from ultrasound_modeling_amd.flat import AdamClip, FlatParams
from ultrasound_modeling_amd.schedules import PiecewiseConstantDecay

SCRIPT_SCHEDULE = ([10000, 20000, 40000, 60000, 80000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])     # TBI_TransUNet.py:927-928


# ---------------------------------------------------------------------------------------------------- the restatement
def script_data_aug(image, label, p, gauss=None):
    """TBI_TransUNet.py:835-875 with the draws ``p`` (TBI_TransUNet.draw) and the unit Gaussian ``gauss`` [H,W,C] injected.
    image [H,W,C] float64, label [H,W] float32 -> (image, label)."""
    image, label = image.copy(), label.copy()
    if p["flip"]:                                                                                              # :840-842
        image, label = np.fliplr(image).copy(), np.fliplr(label).copy()
    if p["reduc"]:                                                                                             # :844-845
        label, image = IO.image_reduc(np.concatenate([np.expand_dims(label, axis=-1), image], axis=2), p["reduc_t"])
    for (r, c, ra, ca) in p["clips"]:                                                                          # :859-860
        label, image = IO.clip(image, label, r, c, ra, ca)
    if p["shift"] is not None:                                                                                 # :869-870
        label, image = IO.shift(image, label, *p["shift"])
    if p["noise"] and gauss is not None:                                                                       # :872-873
        image = image + gauss / 5000
    return image, label


def _off(**kw):
    p = dict(flip=False, reduc=False, reduc_t=0, clips=[], shift=None, noise=False, seed=0)
    p.update(kw)
    return p


class _Counting(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.n = 0

    def randint(self, a, b):
        self.n += 1
        return super().randint(a, b)


def _literal_draws(rng):
    """The random.randint calls of TBI_TransUNet.py:835-875 in execution order (clip :780-783 and shift :760-762 draw inside)."""
    r = rng.randint(0, 100000)
    t = rng.randint(0, 100000)
    clips, shift = [], None
    if r % 3:
        box_r = rng.randint(0, 256)
        box_c = rng.randint(0, 80)
        box_ra = rng.randint(20, 40)
        box_ca = rng.randint(10, 20)
        clips.append((box_r, box_c, box_ra, box_ca))
    if t % 2:
        sr = rng.randint(0, 30)
        sc = rng.randint(0, 12)
        direction = rng.randint(0, 1)
        shift = (sr, sc, direction)
    return dict(flip=bool(r % 2), reduc=r % 5 != 0, reduc_t=r % 5, clips=clips, shift=shift, noise=bool(t % 3))


# ---------------------------------------------------------------------------------------------------- draw
def test_draw_equals_the_scripts_randint_calls():
    seen = set()
    for seed in range(1000):
        a, b = _Counting(seed), _Counting(seed)
        p = T.draw(a)
        want = _literal_draws(b)
        for k in ("flip", "reduc", "reduc_t", "clips", "shift", "noise"):
            assert p[k] == want[k], (seed, k)
        assert isinstance(p["flip"], bool) and isinstance(p["noise"], bool)
        assert len(p["clips"]) <= 1
        assert a.n == b.n == 2 + 4 * len(p["clips"]) + 3 * (p["shift"] is not None), seed
        assert a.randint(0, 10 ** 9) == b.randint(0, 10 ** 9), seed          # the generator is left where the script leaves it
        assert 0 <= p["seed"] < 2 ** 63
        seen.add((p["flip"], p["reduc"], bool(p["clips"]), p["shift"] is not None, p["noise"]))
    assert len(seen) == 32                                                   # every combination of the five flags occurs


def test_draw_differs_from_dataaugs_draw():
    """DataAugs.draw clips r % 3 boxes and reduces when r % 3; the script clips one box and reduces when r % 5."""
    from ultrasound_modeling_amd import DataAugs
    diff = 0
    for seed in range(50):
        p, q = T.draw(random.Random(seed)), DataAugs.draw(random.Random(seed))
        assert "flip" not in q
        diff += (p["reduc"] != q["reduc"]) or len(p["clips"]) != len(q["clips"])
    assert diff > 0


# ---------------------------------------------------------------------------------------------------- the restatement, pinned
def _pattern(H, W, C=2):
    base = (10 * np.arange(H)[:, None] + np.arange(W)[None, :] + 1).astype(np.float64)
    image = np.stack([base * (-1) ** k * (k + 1) for k in range(C)], axis=-1)
    return image, base.astype(np.float32) / 100


def test_flip_alone_is_exact():
    rng = np.random.default_rng(0)
    image = rng.standard_normal((7, 5, 3))
    label = rng.random((7, 5)).astype(np.float32)
    assert not np.array_equal(image, image[:, ::-1]) and not np.array_equal(label, label[:, ::-1])
    xo, yo = script_data_aug(image, label, _off(flip=True))
    np.testing.assert_array_equal(xo, image[:, ::-1])
    np.testing.assert_array_equal(yo, label[:, ::-1])
    np.testing.assert_array_equal(xo[:, 0], image[:, -1])
    xo, yo = script_data_aug(image, label, _off())
    np.testing.assert_array_equal(xo, image)
    np.testing.assert_array_equal(yo, label)


@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_image_reduc_count_is_inert(t):
    """imageReduc(., r % 5) (:845): the dilation never fires (:815), so every count zeroes the image where the label is 0."""
    rng = np.random.default_rng(t)
    image = rng.standard_normal((16, 12, 4))
    label = rng.random((16, 12)).astype(np.float32) * 2
    label[rng.random((16, 12)) < 0.3] = 0.0
    label[3, 4] = 0.05                                                       # < 0.1 (the mask's threshold) but not 0: kept
    lo, io = IO.image_reduc(np.concatenate([label[..., None], image], axis=2), t)
    np.testing.assert_array_equal(lo, label)
    np.testing.assert_array_equal(io, np.where(label[..., None] == 0, 0.0, image))
    assert np.all(io[3, 4] == image[3, 4])


def test_flip_then_clip_known_answer():
    image, label = _pattern(3, 4)
    # flipped channel 0: [[4,3,2,1],[14,13,12,11],[24,23,22,21]]; box (1,1,1,1) covers i = 1, j = 1 of the FLIPPED image
    xo, yo = script_data_aug(image, label, _off(flip=True, clips=[(1, 1, 1, 1)]))
    want = np.array([[4, 3, 2, 1], [14, 0, 12, 11], [24, 23, 22, 21]], dtype=np.float64)
    np.testing.assert_array_equal(xo[..., 0], want)
    np.testing.assert_array_equal(xo[..., 1], -2 * want)
    np.testing.assert_array_equal(yo, (want / 100).astype(np.float32))


@pytest.mark.parametrize("direction, want", [
    (1, [[13, 12, 11, 0], [23, 22, 21, 0], [0, 0, 0, 0]]),       # out[i, j] = flipped[i + 1, j + 1]; last row / column stay 0
    (0, [[0, 0, 0, 0], [0, 4, 3, 0], [0, 0, 0, 0]]),             # out[i, j] = flipped[i - 1, j - 1]
])
def test_flip_then_shift_known_answer(direction, want):
    image, label = _pattern(3, 4)
    xo, yo = script_data_aug(image, label, _off(flip=True, shift=(1, 1, direction)))
    want = np.array(want, dtype=np.float64)
    np.testing.assert_array_equal(xo[..., 0], want)
    np.testing.assert_array_equal(xo[..., 1], -2 * want)
    np.testing.assert_array_equal(yo.astype(np.float32), (want / 100).astype(np.float32))


def test_flip_then_reduc_reads_the_flipped_label():
    image, label = _pattern(2, 3, C=1)
    label[0, 0] = 0.0                                                         # after the flip this zero sits at column 2
    xo, yo = script_data_aug(image, label, _off(flip=True, reduc=True, reduc_t=3))
    np.testing.assert_array_equal(xo[..., 0], [[3, 2, 0], [13, 12, 11]])
    np.testing.assert_array_equal(yo, label[:, ::-1])


# ---------------------------------------------------------------------------------------------------- C ABI
def test_aug_sample_layout():
    from ultrasound_modeling_amd._lib import AugSample
    assert ctypes.sizeof(AugSample) == 72
    assert AugSample.do_flip.offset == 60 and AugSample.seed.offset == 64
    assert not hasattr(AugSample, "reserved")


def test_sample_table_carries_the_flip():
    from ultrasound_modeling_amd import DataAugs
    from ultrasound_modeling_amd._lib import AugSample
    params = [_off(flip=True), _off(), T.draw(random.Random(1))]
    raw = DataAugs._sample_table(params, "cpu").numpy().tobytes()
    arr = (AugSample * 3).from_buffer_copy(raw)
    assert [s.do_flip for s in arr] == [1, 0, int(params[2]["flip"])]
    q = DataAugs.draw(random.Random(1))                                       # DataAugs' draws keep today's table: do_flip 0
    assert AugSample.from_buffer_copy(DataAugs._sample_table([q], "cpu").numpy().tobytes()).do_flip == 0


# ---------------------------------------------------------------------------------------------------- Dataset draw hook
def _raw(n, h=8, w=6, c=10):
    rng = np.random.default_rng(n)
    return rng.random((n, 1, h, w, c + 2))


@pytest.mark.parametrize("fix", [False, True])
def test_dataset_draws_the_scripts_augmentation(monkeypatch, fix):
    from ultrasound_modeling_amd import Dataset_2
    calls = []
    monkeypatch.setattr(Dataset_2, "dataAug_batch", lambda x, y, params, num_classes: calls.append((x, y, params, num_classes)) or (x, y))
    raw = _raw(5)
    ds = T.Dataset(train_data=raw, val_data=raw[:2], device="cpu")
    assert ds.num_class == ds.num_classes == 3 and (ds.height, ds.width, ds.channel) == (8, 6, 10)
    random.seed(7)
    x, y, term = ds.next_train(3, fix=fix)
    assert not term and ds.idx_tr == (0 if fix else 3)
    rng = random.Random(7)
    assert calls[-1][2] == [T.draw(rng) for _ in range(3)] and calls[-1][3] == 3
    np.testing.assert_array_equal(x.numpy(), raw[:3, 0, :, :, 1:-1])
    if not fix:
        x, y, term = ds.next_train(3)                                         # short batch: x[-1-B:-1] (Dataset_2.py:103-104)
        assert term and ds.idx_tr == 0
        np.testing.assert_array_equal(x.numpy(), raw[-4:-1, 0, :, :, 1:-1])
        np.testing.assert_array_equal(y.numpy(), raw[-4:-1, 0, :, :, 0].astype(np.float32))
    base = Dataset_2.Dataset(train_data=raw, val_data=raw[:2], device="cpu")
    random.seed(7)
    base.next_train(3)
    rng = random.Random(7)
    assert calls[-1][2] == [Dataset_2.draw(rng) for _ in range(3)]           # Dataset_2 keeps DataAugs' draws


# ---------------------------------------------------------------------------------------------------- training control flow
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.kernel = nn.Parameter(torch.randn(5, 3))
        self.bias = nn.Parameter(torch.randn(3))


class _StubNet:
    def __init__(self, adamw=False):
        torch.manual_seed(0)
        self.device = torch.device("cpu")
        self.learning_rate, self.weight_decay = 1e-3, 1e-4
        self.optimizer = AdamClip(FlatParams(_Tiny(), "cpu"), lr=1e-3, weight_decay=1e-4 if adamw else None)
        self.steps = 0

    def step(self, x, y, train=False):
        assert train
        self.steps += 1
        return torch.tensor(0.25 * self.steps), torch.full((1, 2, 2, 3), 0.5)


class _StubData:
    def next_train(self, batch_size):
        return torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), True       # one step per epoch


class _StubMetrics:
    made = []

    def __init__(self, num_classes=3, round=True, device=None):
        assert num_classes == 3 and round
        self.updates, self.resets = 0, 0
        _StubMetrics.made.append(self)

    def update_state(self, y, p):
        self.updates += 1

    def result(self):
        return dict(precision=0.5, recall=0.5, f1=0.5, c2_precision=0.0, c2_recall=0.0, c2_f1=float("nan"), mean_iou=0.25)

    def reset_states(self):
        self.resets += 1


def _fields(t):
    t = t.numpy()
    n = int(t[0])
    return n, t[1:n].tolist(), t[16:16 + n].view(np.float32), t[32:32 + n].view(np.float32)


@pytest.fixture
def stubbed(monkeypatch):
    tested = []
    monkeypatch.setattr(T, "test", lambda net, dataset, epoch: tested.append(epoch) or 0.5)
    monkeypatch.setattr(T, "SegMetrics", _StubMetrics)
    monkeypatch.setattr(T, "history", [])
    _StubMetrics.made = []
    return tested


def test_training_tests_every_fifth_epoch_from_zero(stubbed):
    net = _StubNet()
    steps = T.training(net, _StubData(), epochs=11, batch_size=16)
    assert stubbed == [0, 5, 10]
    assert steps == net.steps == 11
    assert [h["epoch"] for h in T.history] == list(range(11)) and all(h["phase"] == "train" for h in T.history)
    assert [h["loss"] for h in T.history] == [0.25 * (e + 1) for e in range(11)]
    m, = _StubMetrics.made
    assert m.updates == 11 and m.resets == 11                                 # updated every step, reset after every epoch


def test_training_keeps_the_fixed_rate_by_default(stubbed):
    net = _StubNet()
    T.training(net, _StubData(), epochs=6, batch_size=16)
    assert not net.optimizer.scheduled and net.optimizer.sched_dev is None
    assert net.optimizer.current_learning_rate() == 1e-3 and net.learning_rate == 1e-3


@pytest.mark.parametrize("adamw", [False, True])
def test_training_schedule_installs_the_scripts_rates(stubbed, adamw):
    net = _StubNet(adamw=adamw)
    T.training(net, _StubData(), epochs=1, batch_size=16, schedule=True)
    s = PiecewiseConstantDecay(*SCRIPT_SCHEDULE)
    assert T.reference_schedule() == s
    n, b, lr, wd = _fields(net.optimizer.sched_dev)
    assert n == 6 and b == SCRIPT_SCHEDULE[0]
    assert lr.tobytes() == (1e-3 * s).values.tobytes()
    assert wd.tobytes() == ((1e-4 * s).values.tobytes() if adamw else np.zeros(6, np.float32).tobytes())
    assert net.learning_rate == 1e-3 * s
    assert (net.weight_decay == 1e-4 * s) if adamw else net.weight_decay == 1e-4
    for step, piece in ((0, 0), (10000, 0), (10001, 1), (80001, 5)):
        net.optimizer.step_dev.fill_(step)
        assert net.optimizer.current_learning_rate() == float((1e-3 * s).values[piece]), step
