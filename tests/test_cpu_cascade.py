"""The brain-mask cascade without a GPU: the two entry points of csrc/cascade.hip (usseg_cascade_gate, usseg_cascade_maps) reject bad
arguments with the library's error code and message before anything is launched, and the host side of TBIEvaluator.Polar_Model splits
the reference's test-data layout and pads the last batch without touching the caller's array."""
import numpy as np
import pytest


def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L.load()


def _gate_args(**kw):
    a = dict(probs=16, C_mask=2, M=64, x=16, ldx=16, x_gated=32, mask=48, stream=None)
    a.update(kw)
    return list(a.values())


def _maps_args(**kw):
    a = dict(probs=16, C=3, M=64, prob_map=32, bleed_prob=48, stream=None)
    a.update(kw)
    return list(a.values())


def test_cascade_gate_rejects_null_pointers():
    lib = _lib()
    for name in ("probs", "x", "x_gated"):
        assert lib.usseg_cascade_gate(*_gate_args(**{name: None})) == -1, name
        assert b"cascade_gate: null pointer" in lib.usseg_last_error()


@pytest.mark.parametrize("bad", [dict(ldx=0), dict(ldx=-8), dict(ldx=12), dict(ldx=4), dict(M=0), dict(M=-1)])
def test_cascade_gate_rejects_bad_geometry(bad):
    lib = _lib()
    assert lib.usseg_cascade_gate(*_gate_args(**bad)) == -1
    assert b"cascade_gate: bad geometry" in lib.usseg_last_error()


@pytest.mark.parametrize("c", [1, 5, 0, -3])
def test_cascade_gate_rejects_class_counts_outside_2_to_4(c):
    lib = _lib()
    assert lib.usseg_cascade_gate(*_gate_args(C_mask=c)) == -1
    assert b"cascade_gate: C_mask must be 2..4" in lib.usseg_last_error()


@pytest.mark.parametrize("bad", [dict(x=24), dict(x_gated=40), dict(x=20, x_gated=20)])
def test_cascade_gate_rejects_misaligned_rows(bad):
    lib = _lib()
    assert lib.usseg_cascade_gate(*_gate_args(**bad)) == -1
    assert b"cascade_gate: x and x_gated must be 16-byte aligned" in lib.usseg_last_error()


def test_cascade_maps_rejects_bad_arguments():
    lib = _lib()
    for name in ("probs", "prob_map", "bleed_prob"):
        assert lib.usseg_cascade_maps(*_maps_args(**{name: None})) == -1, name
        assert b"cascade_maps: null pointer" in lib.usseg_last_error()
    for c in (2, 4, 1):
        assert lib.usseg_cascade_maps(*_maps_args(C=c)) == -1, c
        assert b"cascade_maps: C must be 3" in lib.usseg_last_error()
    for m in (0, -5):
        assert lib.usseg_cascade_maps(*_maps_args(M=m)) == -1, m
        assert b"cascade_maps: bad geometry" in lib.usseg_last_error()


# ------------------------------------------------------------------------------------------------ the host side of Polar_Model
def _data(N, seed=0):
    """The reference's test-data layout [N, 1, 256, 80, 12]: channel 0 the label, 1..10 the input, 11 the B-mode image (float64)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, 1, 256, 80, 12))
    d[..., 0] = rng.integers(0, 3, (N, 1, 256, 80))
    return d


def test_preprocess_splits_the_reference_layout():
    from ultrasound_modeling_amd.TBIEvaluator import preProcess1
    d = _data(3)
    keep = d.copy()
    x, label, bmode = preProcess1(d, (256, 80))
    assert x.shape == (3, 256, 80, 10) and x.dtype == np.float32 and x.flags.c_contiguous
    assert label.shape == bmode.shape == (3, 256, 80)
    for i in range(3):          # the reference's preProcess1 (image_num = i): x = data[i, ..., 1:11], y = data[i, ..., 0], bMode = data[i, ..., 11]
        assert np.array_equal(x[i], d[i, 0, :, :, 1:11].astype(np.float32))
        assert np.array_equal(label[i], d[i, 0, :, :, 0])
        assert np.array_equal(bmode[i], -d[i, 0, :, :, 11])
    x[:] = 0
    label[:] = 7
    bmode[:] = 7
    assert np.array_equal(d, keep)           # new arrays: nothing written through to the caller's data


def test_preprocess_rejects_other_layouts():
    from ultrasound_modeling_amd.TBIEvaluator import preProcess1
    with pytest.raises(ValueError):
        preProcess1(np.zeros((2, 1, 256, 80, 11)), (256, 80))
    with pytest.raises(ValueError):
        preProcess1(np.zeros((2, 1, 128, 80, 12)), (256, 80))
    x, _, _ = preProcess1(np.zeros((2, 4, 64, 80, 12)), (256, 80))       # any d1*d2*d3 == H*W
    assert x.shape == (2, 256, 80, 10)


def test_batches_pad_the_last_batch_with_zero_images():
    from ultrasound_modeling_amd.TBIEvaluator import batches, preProcess1
    d = _data(19, seed=1)
    keep = d.copy()
    x, _, _ = preProcess1(d, (256, 80))
    got = batches(x, 16)
    assert [(lo, n) for lo, n, _ in got] == [(0, 16), (16, 3)]
    for lo, n, xb in got:
        assert xb.shape == (16, 256, 80, 10) and xb.dtype == np.float32 and xb.flags.c_contiguous
        assert np.array_equal(xb[:n], x[lo:lo + n])
        assert not xb[n:].any()
    assert [(lo, n) for lo, n, _ in batches(x[:16], 16)] == [(0, 16)]
    assert [(lo, n) for lo, n, _ in batches(x[:5], 2)] == [(0, 2), (2, 2), (4, 1)]
    assert np.array_equal(d, keep)
