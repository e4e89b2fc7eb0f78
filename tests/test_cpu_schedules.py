"""Learning-rate / weight-decay schedules on the host side: Keras' PiecewiseConstantDecay piece rule and
the float32 bits of ``c * schedule``, argument validation, the device table ``flat.AdamClip`` builds from a schedule and a weight
decay (on a CPU FlatParams: no kernel runs), the argument checks of the new C entry points (rejected before any launch), and the
plateau rule of ``TBI_ResNest.training``."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from ultrasound_modeling_amd import TBI_ResNest
from ultrasound_modeling_amd.flat import AdamClip, FlatParams
from ultrasound_modeling_amd.schedules import PiecewiseConstantDecay

MAIN_NUMPY = ([2000, 4000, 8000, 10000, 15000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])        # MainNumpy.py:83-84
MAIN_PARALLEL = ([10000, 20000, 40000, 60000, 80000], [1e-0, 3e-1, 1e-1, 3e-2, 1e-2, 3e-3])   # MainParallel.py:74-75


# ---------------------------------------------------------------------------------------------------- the piece rule
@pytest.mark.parametrize("x, piece", [(0, 0), (2000, 0), (2001, 1), (4000, 1), (4001, 2), (15000, 4), (15001, 5), (10 ** 6, 5)])
def test_keras_piece_rule(x, piece):
    s = PiecewiseConstantDecay(*MAIN_NUMPY)
    assert s.piece(x) == piece
    assert s(x) == np.float32(MAIN_NUMPY[1][piece]) and s(x).dtype == np.float32


def test_first_piece_covers_boundary_plus_one_updates():
    s = PiecewiseConstantDecay(*MAIN_NUMPY)
    assert sum(1 for x in range(3000) if s(x) == np.float32(1.0)) == 2001


# ---------------------------------------------------------------------------------------------------- c * schedule bits
@pytest.mark.parametrize("ref", [MAIN_NUMPY, MAIN_PARALLEL])
@pytest.mark.parametrize("c", [1e-2, 1e-3, 1e-4])
def test_constant_times_schedule_is_one_float32_product_per_piece(ref, c):
    s = PiecewiseConstantDecay(*ref)
    want = (torch.tensor(c, dtype=torch.float32) * torch.tensor(ref[1], dtype=torch.float32)).numpy()   # TF: fl32(c) * fl32(v)
    for cs in (c * s, s * c):
        assert cs.boundaries == s.boundaries
        assert cs.values.dtype == np.float32 and cs.values.tobytes() == want.tobytes()
        for x in (0, ref[0][0], ref[0][0] + 1, ref[0][-1], ref[0][-1] + 1):
            assert cs(x).tobytes() == want[s.piece(x)].tobytes()


def test_reference_learning_rate_bits():
    """1e-2 * schedule of MainNumpy.py:86, pinned as float32 bit patterns."""
    s = 1e-2 * PiecewiseConstantDecay(*MAIN_NUMPY)
    assert s.values.view(np.int32).tolist() == [0x3C23D70A, 0x3B449BA6, 0x3A83126F, 0x399D4951, 0x38D1B717, 0x37FBA882]


@pytest.mark.parametrize("b, v, err", [
    ([1, 2], [1.0, 2.0], ValueError),                       # len(v) != len(b) + 1
    ([1, 2], [1.0, 2.0, 3.0, 4.0], ValueError),
    ([2, 2], [1.0, 2.0, 3.0], ValueError),                  # not strictly increasing
    ([3, 1], [1.0, 2.0, 3.0], ValueError),
    ([-1], [1.0, 2.0], ValueError),                         # outside the device counter's range
    ([2 ** 31], [1.0, 2.0], ValueError),
    ([1.5], [1.0, 2.0], TypeError),                         # steps are integers
    ([True], [1.0, 2.0], TypeError),
    ([1], [1.0, float("nan")], ValueError),
    ([1], [1.0, float("inf")], ValueError),
    (list(range(16)), [1.0] * 17, ValueError),              # 17 pieces > USSEG_SCHED_MAX_PIECES
])
def test_schedule_argument_validation(b, v, err):
    with pytest.raises(err):
        PiecewiseConstantDecay(b, v)


def test_sixteen_pieces_accepted_and_scalar_only_products():
    s = PiecewiseConstantDecay(list(range(15)), [float(i) for i in range(16)])
    assert s(0) == 0.0 and s(15) == 15.0
    with pytest.raises(TypeError):
        s * "2"
    with pytest.raises(TypeError):
        s * s


# ---------------------------------------------------------------------------------------------------- the optimiser's table (CPU)
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.kernel = nn.Parameter(torch.randn(5, 3))
        self.bias = nn.Parameter(torch.randn(3))
        self.gamma = nn.Parameter(torch.randn(7))


def _opt(**kw):
    torch.manual_seed(0)
    return AdamClip(FlatParams(_Tiny(), "cpu"), **kw)


def _fields(t):
    t = t.numpy()
    n = int(t[0])
    return n, t[1:n].tolist(), t[16:16 + n].view(np.float32), t[32:32 + n].view(np.float32)


def test_default_optimizer_keeps_the_fixed_rate_path():
    o = _opt(lr=1e-3)
    assert not o.scheduled and o.sched_dev is None and o.decay_mask is None
    assert set(o.state_dict()) == {"__adam_m__", "__adam_v__", "__adam_step__"}
    assert len(o.state_tensors()) == 4
    assert o.current_learning_rate() == 1e-3


def test_table_of_schedule_and_decay():
    s = PiecewiseConstantDecay(*MAIN_NUMPY)
    o = _opt(lr=1e-2 * s, weight_decay=1e-4 * s)
    n, b, lr, wd = _fields(o.sched_dev)
    assert n == 6 and b == MAIN_NUMPY[0]
    assert lr.tobytes() == (1e-2 * s).values.tobytes() and wd.tobytes() == (1e-4 * s).values.tobytes()
    assert "__adam_sched__" in o.state_dict() and len(o.state_tensors()) == 6
    for x, piece in ((0, 0), (2000, 0), (2001, 1), (15001, 5)):
        o.step_dev.fill_(x)
        assert o.current_learning_rate() == float((1e-2 * s).values[piece])


def test_table_merges_different_boundaries():
    o = _opt(lr=PiecewiseConstantDecay([5], [1.0, 2.0]), weight_decay=PiecewiseConstantDecay([3, 7], [0.1, 0.2, 0.3]))
    n, b, lr, wd = _fields(o.sched_dev)
    assert n == 4 and b == [3, 5, 7]
    assert lr.tolist() == [1.0, 1.0, 2.0, 2.0]
    assert wd.tolist() == np.float32([0.1, 0.2, 0.2, 0.3]).tolist()
    with pytest.raises(ValueError):
        _opt(lr=PiecewiseConstantDecay(list(range(0, 20, 2)), [1.0] * 11), weight_decay=PiecewiseConstantDecay(list(range(1, 20, 2)), [1.0] * 11))


def test_float_decay_alone_uses_a_one_piece_table():
    o = _opt(lr=1e-3, weight_decay=1e-4)
    n, b, lr, wd = _fields(o.sched_dev)
    assert (n, b) == (1, []) and lr[0] == np.float32(1e-3) and wd[0] == np.float32(1e-4)


def test_decay_exclude_mask():
    o = _opt(lr=1e-3, weight_decay=1e-4, decay_exclude=[r"bias$", "gamma"])
    f = o.flat
    mask = o.decay_mask
    assert mask.dtype == torch.uint8 and mask.numel() == f.total
    for name, p, off in zip(f.names, f.params, f.offsets):
        assert bool((mask[off:off + p.numel()] == (0 if name in ("bias", "gamma") else 1)).all()), name
    assert _opt(lr=1e-3, weight_decay=1e-4, decay_exclude=["nothing matches"]).decay_mask is None


def test_set_learning_rate_switches_and_refuses_after_capture():
    o = _opt(lr=1e-3)
    o.set_learning_rate(PiecewiseConstantDecay([1], [1.0, 0.5]))
    assert o.scheduled and _fields(o.sched_dev)[2].tolist() == [1.0, 0.5]
    o.set_weight_decay(0.25)
    assert _fields(o.sched_dev)[3].tolist() == [0.25, 0.25]
    o.mark_captured()
    o.set_learning_rate(2e-3)                        # the table path is part of the graph: it follows
    assert _fields(o.sched_dev)[2].tolist() == [np.float32(2e-3)]
    p = _opt(lr=1e-3)
    p.mark_captured()
    with pytest.raises(RuntimeError):
        p.set_learning_rate(2e-3)                    # a fixed-rate graph could not follow it
    with pytest.raises(ValueError):
        _opt(lr=float("nan"))


def test_state_dict_round_trip_of_the_table():
    s = PiecewiseConstantDecay([2, 4], [1.0, 0.5, 0.25])
    a = _opt(lr=1e-3 * s, weight_decay=1e-4)
    a.step_dev.fill_(3)
    d = a.state_dict()
    b = _opt(lr=1e-3)                                  # a float model loads a scheduled checkpoint: it follows the saved table
    b.load_state_dict(d)
    assert b.scheduled and torch.equal(b.sched_dev, a.sched_dev) and int(b.step_dev) == 3
    assert b.lr == 1e-3 * s and b.current_learning_rate() == a.current_learning_rate()
    c = _opt(lr=1e-3 * s)
    old = {k: v for k, v in _opt(lr=1e-3).state_dict().items()}      # an old-format checkpoint keeps the constructor's schedule
    c.load_state_dict(old)
    assert c.lr == 1e-3 * s and c.scheduled


# ---------------------------------------------------------------------------------------------------- C ABI argument checks
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L.load()


def _adamw(**kw):
    a = dict(p=256, g=256, m=256, v=256, n=8, sumsq=256, clip=1.0, lr_t=256, wd_t=256, mask=None, b1=0.9, b2=0.999, eps=1e-7, stream=None)
    a.update(kw)
    return list(a.values())


def test_adamw_step_rejects_null_pointers():
    lib = _lib()
    for name in ("p", "g", "m", "v", "lr_t", "wd_t"):
        assert lib.usseg_adamw_step(*_adamw(**{name: None})) == -1, name
        assert b"adamw_step: null pointer" in lib.usseg_last_error()
    assert lib.usseg_adamw_step(*_adamw(sumsq=None)) == -1
    assert b"needs sumsq" in lib.usseg_last_error()


@pytest.mark.parametrize("name", ["p", "g", "m", "v"])
def test_adamw_step_rejects_misaligned_vectors(name):
    lib = _lib()
    assert lib.usseg_adamw_step(*_adamw(**{name: 260})) == -1
    assert b"16-byte aligned" in lib.usseg_last_error()


def test_adamw_step_rejects_negative_n_and_misaligned_mask():
    lib = _lib()
    assert lib.usseg_adamw_step(*_adamw(n=-1)) == -1
    assert b"n < 0" in lib.usseg_last_error()
    assert lib.usseg_adamw_step(*_adamw(mask=258)) == -1
    assert b"decay_mask must be 4-byte aligned" in lib.usseg_last_error()
    assert lib.usseg_adamw_step(*_adamw(n=0, sumsq=None, clip=0.0)) == 0       # nothing to do: no launch


def test_sched_advance_entry_points_reject_bad_arguments():
    lib = _lib()
    ok = dict(step=256, sched=256, lr_t=256, wd_t=256)
    for name in ok:
        a = dict(ok, **{name: None})
        assert lib.usseg_sched_advance(a["step"], a["sched"], a["lr_t"], a["wd_t"], 0.9, 0.999, None) == -1, name
        assert b"sched_advance: null pointer" in lib.usseg_last_error()
        assert lib.usseg_sumsq_sched_advance(256, 64, 256, a["step"], a["sched"], a["lr_t"], a["wd_t"], 0.9, 0.999, None) == -1, name
        assert b"sumsq_sched_advance: null pointer" in lib.usseg_last_error()
    for g, n in ((None, 64), (260, 64), (256, 0)):
        assert lib.usseg_sumsq_sched_advance(g, n, 256, 256, 256, 256, 256, 0.9, 0.999, None) == -1
        assert b"sumsq_sched_advance: bad args" in lib.usseg_last_error()


# ---------------------------------------------------------------------------------------------------- TBI_ResNest.training
class _StubOptimizer:
    def __init__(self):
        self.calls = []

    def set_learning_rate(self, lr):
        self.calls.append(lr)


class _StubNet:
    def __init__(self, lr):
        self.learning_rate = lr
        self.optimizer = _StubOptimizer()
        self.steps = 0

    def step(self, x, y, train=False):
        assert train
        self.steps += 1
        return torch.zeros(2, 2), torch.tensor(0.5), None

    def _loss_total(self, loss_map):
        return loss_map.sum()


class _StubData:
    def next_train(self, batch_size):
        return None, None, True                       # one step per epoch


@pytest.mark.parametrize("live_lr", [False, True])
def test_resnest_training_plateau_rule(monkeypatch, live_lr):
    f1 = iter([0.5, 0.6, 0.4, 0.3, 0.9])
    tested = []

    def fake_test(net, dataset, epoch):
        tested.append(epoch)
        return next(f1)
    monkeypatch.setattr(TBI_ResNest, "test", fake_test)
    net = _StubNet(lr=1e-4)
    steps = TBI_ResNest.training(net, _StubData(), epochs=30, batch_size=2, live_lr=live_lr)
    # epochs 0, 3 test (0.5, 0.6: no drop); epoch 6: 0.4 < 0.6 -> 2e-5; epoch 9: 0.3 < 0.4 -> 4e-6 < 1e-5: stop before epoch 10
    assert tested == [0, 3, 6, 9]
    assert steps == net.steps == 10
    assert net.learning_rate == pytest.approx(1e-4 / 25)
    assert net.optimizer.calls == ([pytest.approx(2e-5), pytest.approx(4e-6)] if live_lr else [])


def test_resnest_training_compares_against_the_previous_epoch(monkeypatch):
    """f1prev follows f1cur every epoch, so a drop is seen once: the epochs between tests compare a value with itself."""
    f1 = iter([0.5, 0.4, 0.4, 0.4])
    monkeypatch.setattr(TBI_ResNest, "test", lambda net, dataset, epoch: next(f1))
    net = _StubNet(lr=1.0)
    TBI_ResNest.training(net, _StubData(), epochs=10, batch_size=2, live_lr=True)
    assert net.optimizer.calls == [pytest.approx(0.2)]


# ---------------------------------------------------------------------------------------------------- MainNumpy schedule
class _StubModel:
    def __init__(self, **kw):
        self.optimizer = _opt(**kw)
        self.learning_rate, self.weight_decay = 1e-3, 1e-4


@pytest.mark.parametrize("adamw", [False, True])
def test_main_numpy_installs_the_reference_schedule(adamw):
    from ultrasound_modeling_amd.MainNumpy import install_schedule, reference_schedule
    net = _StubModel(lr=1e-3, weight_decay=1e-4 if adamw else None)
    install_schedule(net)
    s = reference_schedule()
    n, b, lr, wd = _fields(net.optimizer.sched_dev)
    assert n == 6 and b == MAIN_NUMPY[0] and lr.tobytes() == (1e-2 * s).values.tobytes()
    assert wd.tobytes() == ((1e-4 * s).values.tobytes() if adamw else np.zeros(6, np.float32).tobytes())
    assert net.learning_rate == 1e-2 * s
