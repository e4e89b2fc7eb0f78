"""CPU tests of the EMA / SWA weight averaging: the NumPy restatement (tests/average_restatement.py) pinned by known
answers, the host-side validation and the ``--average`` strings, the exported symbols and their argument checks, and that an optimiser
without ``average`` keeps the state it had."""
import numpy as np
import pytest
import torch

import average_restatement as A


# ------------------------------------------------------------------------------------------------ the restatement, by known answers
def test_swa_over_snapshots_is_their_arithmetic_mean():
    rng = np.random.default_rng(0)
    start, period = 5, 3
    avg = rng.standard_normal(257)          # the initial average: the first snapshot must replace it
    snaps = []
    for t in range(1, 30):
        p = rng.standard_normal(257)
        c = A.coeff(A.SWA, t, start=start, period=period)
        if c != 0:
            snaps.append(p)
            c = 1.0 / len(snaps)            # the fp64 coefficient: this test is about the rule, not about fp32
        avg = avg + c * (p - avg) if c not in (0, 1) else (p.copy() if c == 1 else avg)
    assert len(snaps) == 9 == A.snapshots_so_far(A.SWA, 29, start, period)
    mean = np.mean(snaps, axis=0)
    assert np.max(np.abs(avg - mean) / np.abs(mean)) <= 1e-12


def test_swa_fp32_coefficients_are_the_rounded_reciprocals():
    for k in range(40):
        assert A.coeff(A.SWA, 5 + 3 * k, start=5, period=3) == np.float32(1.0) / np.float32(k + 1)


def test_ema_of_a_constant_stays_the_constant_exactly():
    p = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    avg = p.copy()
    for t in range(1, 50):
        for dyn in (False, True):
            c = A.coeff(A.EMA, t, decay=0.99, dynamic_decay=dyn)
            assert 0 < c < 1
            avg = A.update32(avg, p, c)
            assert np.array_equal(avg.view(np.int32), p.view(np.int32))
            assert np.array_equal(A.update64(avg, p, c), p.astype(np.float64))


def test_dynamic_decay_sequence():
    d = np.float32(0.9)
    for t in range(1, 31):
        want = min(d, np.float32(1 + t) / np.float32(10 + t))
        assert A.coeff(A.EMA, t, decay=0.9, dynamic_decay=True) == np.float32(1) - want
        assert abs(float(want) - min(0.9, (1 + t) / (10 + t))) < 1e-7
    assert A.coeff(A.EMA, 1, decay=0.9, dynamic_decay=True) == np.float32(1) - np.float32(2) / np.float32(11)      # (1+t)/(10+t) rules early
    assert A.coeff(A.EMA, 100, decay=0.9, dynamic_decay=True) == np.float32(1) - d                                   # the decay rules late
    assert A.coeff(A.EMA, 7, decay=0.9) == np.float32(1) - d


def test_until_start_the_average_tracks_the_weights_exactly():
    rng = np.random.default_rng(2)
    avg = rng.standard_normal(64).astype(np.float32)
    for t in range(0, 5):
        p = rng.standard_normal(64).astype(np.float32)
        c = A.coeff(A.EMA, t, decay=0.5, start=4)
        assert c == 1
        avg = A.update32(avg, p, c)
        assert np.array_equal(avg.view(np.int32), p.view(np.int32))
    assert A.coeff(A.EMA, 5, decay=0.5, start=4) == np.float32(0.5)


def test_swa_coefficient_sequence():
    got = [A.coeff(A.SWA, t, start=5, period=3) for t in range(21)]
    want = [np.float32(0)] * 21
    for k, t in enumerate(range(5, 21, 3)):
        want[t] = np.float32(1) / np.float32(k + 1)
    assert got == want
    assert [t for t in range(21) if got[t] != 0] == [5, 8, 11, 14, 17, 20]
    assert got[5] == 1 and got[8] == np.float32(0.5)


def test_update32_stays_within_the_bound_of_update64():
    rng = np.random.default_rng(3)
    avg, p = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    for c in (np.float32(0.001), np.float32(1) / np.float32(3), np.float32(0.9)):
        err = np.abs(A.update32(avg, p, c).astype(np.float64) - A.update64(avg, p, c))
        assert np.all(err <= A.bound(avg, p))
    assert np.array_equal(A.update32(avg, p, np.float32(0)), avg) and np.array_equal(A.update32(avg, p, np.float32(1)), p)


# ------------------------------------------------------------------------------------------------ host validation and the CLI strings
def test_average_config_fills_the_defaults():
    from ultrasound_modeling_amd.flat import average_config
    assert average_config({"mode": "ema"}) == {"mode": "ema", "decay": 0.999, "dynamic_decay": False, "start_step": 0}
    assert average_config({"mode": "swa", "start": 7, "period": 2}) == {"mode": "swa", "start": 7, "period": 2}
    assert average_config({"mode": "swa"}) == {"mode": "swa", "start": 0, "period": 1}


@pytest.mark.parametrize("bad", [
    {"mode": "mean"}, {}, "ema", {"mode": "ema", "decay": 1.0}, {"mode": "ema", "decay": -0.1}, {"mode": "ema", "decay": float("nan")},
    {"mode": "ema", "decay": 1.0 - 1e-12}, {"mode": "ema", "start_step": -1}, {"mode": "ema", "period": 3}, {"mode": "swa", "period": 0},
    {"mode": "swa", "start": -1}, {"mode": "swa", "start": 1.5}, {"mode": "swa", "decay": 0.5}])
def test_average_config_rejects(bad):
    from ultrasound_modeling_amd.flat import average_config
    with pytest.raises(ValueError):
        average_config(bad)


def test_cli_strings_parse():
    from ultrasound_modeling_amd.flat import parse_average
    assert parse_average("ema:0.999") == {"mode": "ema", "decay": 0.999, "dynamic_decay": False, "start_step": 0}
    assert parse_average("ema:0.9:dynamic") == {"mode": "ema", "decay": 0.9, "dynamic_decay": True, "start_step": 0}
    assert parse_average("swa:100:10") == {"mode": "swa", "start": 100, "period": 10}
    for bad in ("ema", "ema:1.0", "ema:0.9:static", "swa:5", "swa:5:0", "swa:a:b", "mean:1:2", ""):
        with pytest.raises(ValueError):
            parse_average(bad)


def test_descriptor_words_round_trip():
    from ultrasound_modeling_amd import flat, ops
    for cfg in ({"mode": "ema", "decay": 0.75, "dynamic_decay": True, "start_step": 4}, {"mode": "swa", "start": 5, "period": 3}):
        w = flat._average_words(flat.average_config(cfg))
        assert w.dtype == np.int32 and w.size == ops.AVERAGE_WORDS == 5 and w[0] == ops.AVERAGE_MODES[cfg["mode"]]
        assert flat._average_from_words(w) == cfg
    assert w.tolist() == [2, 0, 0, 5, 3]


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbols_are_exported_and_check_their_arguments():
    from ultrasound_modeling_amd import _lib as L
    lib = L.load()
    for name in ("usseg_adamw_avg_step", "usseg_average_update", "usseg_swap_f32"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.usseg_average_update(None, 16, 4, 16, 16, None) == -1
    assert b"average_update: null pointer" in lib.usseg_last_error()
    assert lib.usseg_average_update(16, 20, 4, 16, 16, None) == -1
    assert b"16-byte aligned" in lib.usseg_last_error()
    assert lib.usseg_swap_f32(16, None, 4, None) == -1
    assert b"swap_f32: null pointer" in lib.usseg_last_error()
    assert lib.usseg_swap_f32(1024, 1024 + 16, 8, None) == -1
    assert b"swap_f32: a and b overlap" in lib.usseg_last_error()
    assert lib.usseg_swap_f32(1024, 2048, 0, None) == 0                        # nothing to do, nothing launched
    args = dict(p=16, g=16, m=16, v=16, avg=16, n=4, sumsq=16, clip=0.0, lr_t=16, wd_t=None, mask=None, b1=0.9, b2=0.999, eps=1e-7, step=16,
                desc=16, stream=None)
    for k in ("p", "avg", "lr_t", "step", "desc"):
        assert lib.usseg_adamw_avg_step(*dict(args, **{k: None}).values()) == -1, k
        assert b"adamw_avg_step: null pointer" in lib.usseg_last_error()
    assert lib.usseg_adamw_avg_step(*dict(args, avg=20).values()) == -1
    assert b"must be 16-byte aligned" in lib.usseg_last_error()
    assert lib.usseg_adamw_avg_step(*dict(args, clip=1.0, sumsq=None).values()) == -1
    assert lib.usseg_adamw_avg_step(*dict(args, n=0).values()) == 0           # wd_t and mask may be null; n == 0 launches nothing


# ------------------------------------------------------------------------------------------------ the optimiser without / with average
class _Flat:
    """What ``AdamClip`` needs of ``FlatParams``."""

    def __init__(self, n, device="cpu"):
        self.device, self.total = torch.device(device), n
        self.flat = torch.arange(n, dtype=torch.float32, device=device)
        self.grad = torch.zeros(n, dtype=torch.float32, device=device)
        self.names, self.params, self.offsets = [], [], []


def test_without_average_the_optimiser_keeps_its_state():
    from ultrasound_modeling_amd.flat import AdamClip
    opt = AdamClip(_Flat(16), lr=1e-3, average=None)
    assert set(opt.state_dict()) == {"__adam_m__", "__adam_v__", "__adam_step__"}
    assert opt.avg is None and opt.avg_desc is None and opt.average_state() is None
    assert [t.data_ptr() for t in opt.state_tensors()] == [t.data_ptr() for t in (opt.m, opt.v, opt.step_dev, opt.lr_t_dev)]
    with pytest.raises(ValueError):
        opt.set_average_decay(0.5)
    opt.params_loaded()                     # a no-op


def test_with_average_the_state_carries_it():
    from ultrasound_modeling_amd.flat import AdamClip
    f = _Flat(16)
    opt = AdamClip(f, lr=1e-3, average={"mode": "ema", "decay": 0.5})
    assert torch.equal(opt.avg, f.flat) and opt.avg.data_ptr() != f.flat.data_ptr()
    assert opt.avg_desc.tolist() == [1, int(np.float32(0.5).view(np.int32)), 0, 0, 1]
    assert set(opt.state_dict()) == {"__adam_m__", "__adam_v__", "__adam_step__", "__adam_avg__", "__adam_avg_desc__"}
    assert {t.data_ptr() for t in opt.state_tensors()} >= {opt.avg.data_ptr(), opt.avg_desc.data_ptr()}
    opt.set_average_decay(0.25)
    assert opt.avg_desc[1].item() == int(np.float32(0.25).view(np.int32)) and opt.average_state() == ("ema", 0, 0)
    with pytest.raises(ValueError):
        opt.set_average_decay(1.0)
    f.flat.add_(1.0)                        # weights loaded after construction, before the first step: the average follows them
    opt.params_loaded()
    assert torch.equal(opt.avg, f.flat)
    other = AdamClip(_Flat(16), lr=1e-3, average={"mode": "swa", "start": 2, "period": 2})
    other.load_state_dict(opt.state_dict())             # the saved settings replace the constructor's
    assert other.average == opt.average and torch.equal(other.avg, opt.avg) and torch.equal(other.avg_desc, opt.avg_desc)
    plain = AdamClip(_Flat(16), lr=1e-3).state_dict()   # a checkpoint without an average: it starts from the loaded weights
    other.load_state_dict(plain)
    other.step_dev.fill_(3)                             # (not only because the counter is 0)
    other.flat.flat.mul_(2.0)
    other.params_loaded()
    assert torch.equal(other.avg, other.flat.flat)
    with pytest.raises(ValueError):
        AdamClip(_Flat(16), average={"mode": "swa", "period": 0})
