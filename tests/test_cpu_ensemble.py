"""Ensembles and calibration without a GPU: known answers of the NumPy restatement (tests/ensemble_restatement.py) that the device tests
compare the kernels with, the three new symbols, every argument check of csrc/ensemble.hip (an error code and a message before any launch),
the refusals of the Python surface, and the tuples other code relies on."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ensemble_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("usseg_ensemble_merge", "usseg_ensemble_image_scores", "usseg_calibration_bins")


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ known answers: the merge
def test_identical_members_have_no_mutual_information_and_no_variance():
    p = _softmax(np.random.default_rng(0).standard_normal((2, 3, 5, 3)))
    r = R.merge([p, p, p, p])
    assert np.abs(r["mutual_info"]).max() < 1e-15 and np.abs(r["variance"]).max() < 1e-15
    assert np.allclose(r["entropy"], -(p.astype(np.float64) * np.log(p.astype(np.float64))).sum(-1), rtol=0, atol=1e-15)
    assert np.array_equal(R.mean_f32([p, p, p, p]), p)          # x4 then / 4: exact in binary


def test_two_disagreeing_one_hot_members_give_ln2_twice():
    a = np.zeros((1, 2, 2, 2), np.float32)
    a[..., 0] = 1
    b = 1 - a
    r = R.merge([a, b])
    assert np.allclose(r["entropy"], math.log(2), rtol=0, atol=1e-15)
    assert np.allclose(r["mutual_info"], math.log(2), rtol=0, atol=1e-15)       # the member entropies are 0: p <= 0 contributes 0
    assert np.allclose(r["variance"], 0.25)
    assert np.array_equal(R.mean_f32([a, b]), np.full_like(a, 0.5))


def test_the_flip_is_an_involution_and_unmirrors_along_w():
    rng = np.random.default_rng(1)
    ms = [_softmax(rng.standard_normal((2, 3, 7, 3))) for _ in range(3)]
    twice = R.unflip(R.unflip(ms, 0b101), 0b101)
    assert all(np.array_equal(a, b) for a, b in zip(ms, twice))
    mirrored = [m[:, :, ::-1] for m in ms]
    assert np.array_equal(R.mean_f32(mirrored, 0b111), R.mean_f32(ms, 0))
    got = R.unflip(ms, 0b010)
    assert np.array_equal(got[1][0, 1, 2], ms[1][0, 1, 4]) and got[0] is ms[0]


def test_nan_propagates_and_a_non_positive_term_contributes_nothing():
    p = np.array([[[[0.5, 0.5, 0.0]]]], np.float32)
    q = np.array([[[[np.nan, 0.5, 0.5]]]], np.float32)
    assert np.isclose(R.merge([p])["entropy"][0, 0, 0], math.log(2))
    r = R.merge([p, q])
    assert np.isnan(r["entropy"]).all() and np.isnan(r["mutual_info"]).all() and np.isnan(r["variance"][..., 0]).all()
    assert not np.isnan(r["variance"][..., 1:]).any()
    assert R.plogp(np.array([-0.25, 0.0]))[0] == 0.0 and R.plogp(np.array([-0.25, 0.0]))[1] == 0.0


def test_image_scores_of_a_small_stack():
    mean = np.zeros((2, 1, 3, 3), np.float32)
    mean[0, 0, :, 2] = (0.9, 0.2, 0.4)      # image 0: the last class wins in pixels 0 and 2 (0.4 ties with nothing: the others are 0)
    mean[0, 0, 1, 0] = 0.8
    mean[1] = 1.0 / 3                        # image 1: all equal - the FIRST maximum is class 0, so no pixel counts
    e = np.array([[[1.0, 2.0, 4.0]], [[1.0, 1.0, 1.0]]])
    m = np.array([[[0.5, 0.25, 0.0]], [[0.0, 0.0, 0.125]]])
    s, n, _ = R.image_scores(mean, e, m)
    assert n.tolist() == [2, 0]
    assert np.allclose(s, [[7 / 3, 0.25, 0.5, 2.5], [1.0, 0.125 / 3, 0.125, 0.0]])


# ------------------------------------------------------------------------------------------------ known answers: calibration
def test_a_perfectly_calibrated_input_has_ece_zero():
    # bins = 4; confidences 0.625 (bin 2) and 0.875 (bin 3), exact in binary; 8 pixels at 0.625 with 5 hits, 8 at 0.875 with 7 hits
    probs, y = [], []
    for conf, hits in ((0.625, 5), (0.875, 7)):
        for i in range(8):
            probs.append([conf, 1 - conf])
            y.append([1, 0] if i < hits else [0, 1])
    probs, y = np.array(probs, np.float32).reshape(1, 4, 4, 2), np.array(y, np.float32).reshape(1, 4, 4, 2)
    counts, _, n_valid = R.calibration(probs, y, 4)
    s = R.scores_from_counts(counts)
    assert n_valid == 16 and s["n"].tolist() == [0, 0, 8, 8] and s["n_invalid"] == 0
    assert s["ece"] == 0.0 and s["mce"] == 0.0
    assert np.array_equal(s["confidence"], [0, 0, 0.625, 0.875]) and np.array_equal(s["accuracy"], [0, 0, 0.625, 0.875])


def test_all_confident_and_all_wrong_has_ece_one():
    probs = np.zeros((1, 2, 3, 3), np.float32)
    probs[..., 2] = 1
    y = np.zeros_like(probs)
    y[..., 0] = 1
    counts, brier, _ = R.calibration(probs, y, 15)
    s = R.scores_from_counts(counts)
    assert s["ece"] == 1.0 and s["mce"] == 1.0 and s["n"][14] == 6 and s["brier"] == 2.0 and brier == 6 * 2 * 2.0 ** 24


def test_bin_edges_and_the_last_bin():
    bins = 10
    conf = np.array([k / bins for k in range(bins)] + [1.0], np.float32)           # exactly k / bins (as fp32) and exactly 1.0
    probs = np.stack([conf, 1 - conf], -1).reshape(1, 1, bins + 1, 2)
    y = np.zeros_like(probs)
    y[..., 0] = 1
    counts, _, _ = R.calibration(probs, y, bins, cls=0)
    want = [int(np.float32(c) * np.float32(bins)) for c in conf[:-1]]             # fp32: 0.3f * 10 is 3.0000001 -> 3, 0.7f * 10 -> 7, ...
    want = np.bincount(want + [bins - 1], minlength=bins)                         # 1.0 goes to the LAST bin, not to bin `bins`
    assert counts[0:3 * bins:3].tolist() == want.tolist() and want[bins - 1] == 2
    assert counts[3 * bins + 1] == 0
    assert counts[3 * (bins - 1) + 2] == int(np.rint(np.float32(0.9) * R.Q)) + 2 ** 24


def test_a_nan_and_a_value_above_one_are_invalid_only():
    probs = np.array([[0.5, 0.5], [np.nan, 0.2], [1.5, 0.1], [-0.25, -0.5], [0.75, 0.25]], np.float32).reshape(1, 1, 5, 2)
    y = np.tile(np.array([1, 0], np.float32), (5, 1)).reshape(1, 1, 5, 2)
    for cls in (-1, 0):
        counts, _, n_valid = R.calibration(probs, y, 4, cls=cls)
        assert n_valid == 2 and counts[-1] == 3
        assert counts[0:12:3].sum() == 2 and counts[1:12:3].sum() == 2
    counts, _, n_valid = R.calibration(probs, y, 4, cls=1)       # class 1: 0.5, 0.2, 0.1, (-0.5 invalid), 0.25; no pixel is labelled class 1
    assert n_valid == 4 and counts[-1] == 1 and counts[1:12:3].sum() == 0 and counts[0:12:3].tolist() == [2, 1, 1, 0]


def test_quantisation_rounds_half_to_even():
    conf = np.array([2.0 ** -25, 3 * 2.0 ** -25, 0.5], np.float32)                # x 2^24 = 0.5, 1.5, 2^23: rint -> 0, 2, 2^23
    probs = np.stack([conf, 1 - conf], -1).reshape(1, 1, 3, 2)
    counts, _, _ = R.calibration(probs, np.zeros_like(probs), 1, cls=0)
    assert counts[2] == 0 + 2 + 2 ** 23


# ------------------------------------------------------------------------------------------------ symbols
def test_the_three_symbols_are_declared_listed_and_exported():
    from ultrasound_modeling_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert "#define USSEG_ENSEMBLE_MAX 16" in hdr and _lib.ENSEMBLE_MAX == 16
    assert "#define USSEG_CALIB_MAX_BINS 64" in hdr and _lib.CALIB_MAX_BINS == 64


# ------------------------------------------------------------------------------------------------ argument checks (no launch: no device needed)
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _merge(K=2, C_=3, B=1, H=4, W=4, flip_w=0, members="ok", **ptr):
    L, lib = _lib()
    d = L.EnsembleDesc(B, H, W, C_, K)
    n = max(K, 1)
    arr = (C.c_void_p * n)(*([64] * n))
    if members == "null":
        arr = None
    elif members == "hole":
        arr[n - 1] = None
    a = dict(mean=16, ent=32, mi=48, var=None)
    a.update(ptr)
    return lib.usseg_ensemble_merge(C.byref(d), arr, flip_w, a["mean"], a["ent"], a["mi"], a["var"], None), lib.usseg_last_error()


def test_merge_rejects_null_pointers():
    L, lib = _lib()
    assert lib.usseg_ensemble_merge(None, (C.c_void_p * 1)(64), 0, 16, 32, 48, None, None) == -1
    for kw in (dict(mean=None), dict(ent=None), dict(mi=None), dict(members="null"), dict(members="hole")):
        rc, msg = _merge(**kw)
        assert rc == -1 and b"ensemble_merge: null pointer" in msg, kw


@pytest.mark.parametrize("c", [0, 5, -1])
def test_merge_rejects_class_counts_outside_1_to_4(c):
    rc, msg = _merge(C_=c)
    assert rc == -1 and b"1 <= C <= 4" in msg


@pytest.mark.parametrize("k", [0, 17, -2])
def test_merge_rejects_member_counts_outside_1_to_16(k):
    rc, msg = _merge(K=k)
    assert rc == -1 and b"1 <= K <= 16" in msg


def test_merge_rejects_bad_geometry_and_stray_flip_bits():
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15)):
        rc, msg = _merge(**kw)
        assert rc == -1 and b"ensemble_merge: bad descriptor (B, H, W" in msg, kw
    rc, msg = _merge(K=2, flip_w=0b100)
    assert rc == -1 and b"flip_w" in msg


def test_image_scores_rejects_bad_arguments():
    L, lib = _lib()
    good = dict(mean=16, ent=32, mi=48, scores=64, counts=80)
    for name in good:
        a = dict(good, **{name: None})
        assert lib.usseg_ensemble_image_scores(C.byref(L.EnsembleDesc(1, 4, 4, 3, 1)), *a.values(), None) == -1, name
        assert b"ensemble_image_scores: null pointer" in lib.usseg_last_error()
    assert lib.usseg_ensemble_image_scores(None, *good.values(), None) == -1
    for d in (L.EnsembleDesc(1, 4, 4, 0, 1), L.EnsembleDesc(1, 4, 4, 5, 1), L.EnsembleDesc(0, 4, 4, 3, 1), L.EnsembleDesc(1, 4, 0, 3, 1)):
        assert lib.usseg_ensemble_image_scores(C.byref(d), *good.values(), None) == -1
        assert b"ensemble_image_scores: bad descriptor" in lib.usseg_last_error()


def _calib(B=1, H=4, W=4, C_=3, bins=15, cls=-1, probs=16, y=32, counts=48):
    L, lib = _lib()
    return lib.usseg_calibration_bins(C.byref(L.CalibDesc(B, H, W, C_, bins, cls)), probs, y, counts, None), lib.usseg_last_error()


def test_calibration_rejects_bad_arguments():
    L, lib = _lib()
    assert lib.usseg_calibration_bins(None, 16, 32, 48, None) == -1
    for kw in (dict(probs=None), dict(y=None), dict(counts=None)):
        rc, msg = _calib(**kw)
        assert rc == -1 and b"calibration_bins: null pointer" in msg, kw
    for c in (0, 5):
        rc, msg = _calib(C_=c)
        assert rc == -1 and b"1 <= C <= 4" in msg, c
    for b in (0, 65, -1):
        rc, msg = _calib(bins=b)
        assert rc == -1 and b"1 <= bins <= 64" in msg, b
    for cls, c in ((3, 3), (2, 2), (4, 4), (-2, 3)):
        rc, msg = _calib(cls=cls, C_=c)
        assert rc == -1 and b"cls is -1 or a class below C" in msg, (cls, c)
    for kw in (dict(B=-1), dict(H=-1), dict(W=0)):
        rc, msg = _calib(**kw)
        assert rc == -1 and b"calibration_bins: bad descriptor (B, H" in msg, kw
    assert _calib(B=0)[0] == 0 and _calib(H=0)[0] == 0        # an empty batch: nothing to count, nothing launched


# ------------------------------------------------------------------------------------------------ the Python surface
class _Stub:
    """Enough of a model for the constructor's checks (they read attributes only)."""


def _arch_b(device="cuda:0", img=(64, 64), ch=1, classes=3):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    m = VisionTransformer.__new__(VisionTransformer)
    m.__dict__.update(device=device, img_size=img, input_shape=[img[0], img[1], ch], num_classes=classes)
    return m


def _arch_a(device="cuda:0", img=(64, 64), ch=1, classes=3):
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    m = ResNest.__new__(ResNest)
    m.__dict__.update(device=device, height=img[0], width=img[1], channel=ch, num_class=classes)
    return m


def test_ensemble_constructor_refusals():
    from ultrasound_modeling_amd.ensemble import Ensemble
    with pytest.raises(ValueError, match="takes VisionTransformer"):
        Ensemble(_Stub())
    with pytest.raises(ValueError, match="at least one"):
        Ensemble([])
    for other, what in ((_arch_b(device="cuda:1"), "devices"), (_arch_b(img=(64, 32)), "image sizes"), (_arch_b(ch=2), "input channels"),
                        (_arch_b(classes=2), "class counts"), (_arch_a(classes=2), "class counts")):
        with pytest.raises(ValueError, match=what):
            Ensemble([_arch_b(), other])
    with pytest.raises(ValueError, match="draws > 1"):
        Ensemble(_arch_b(), draws=2)
    with pytest.raises(ValueError, match="draws > 1"):
        Ensemble([_arch_a(), _arch_b()], draws=2)
    with pytest.raises(ValueError, match="draws must be"):
        Ensemble(_arch_a(), draws=0)
    with pytest.raises(ValueError, match="17 members"):
        Ensemble(_arch_a(), draws=17)
    with pytest.raises(ValueError, match="18 members"):
        Ensemble([_arch_b()] * 9, flip=True)


def test_ensemble_member_count_and_geometry():
    from ultrasound_modeling_amd.ensemble import Ensemble, EnsembleOutput
    e = Ensemble([_arch_a(), _arch_a()], flip=True, draws=4)
    assert e.members == 16 and e.num_classes == 3 and e.img_size == (64, 64) and e.input_shape == [64, 64, 1] and e.device == "cuda:0"
    assert Ensemble(_arch_b()).members == 1 and Ensemble([_arch_b(), _arch_a()], flip=True).members == 4
    assert EnsembleOutput._fields == ("probs", "entropy", "mutual_info", "variance", "image_scores", "image_counts")


def test_cascade_takes_an_ensemble_of_arch_b_models_only():
    from ultrasound_modeling_amd.ensemble import Ensemble
    from ultrasound_modeling_amd.TBIEvaluator import Cascade
    c = Cascade(Ensemble([_arch_b(), _arch_b()], flip=True), _arch_b(classes=2))
    assert c.ensemble and c.img_size == (64, 64) and c.in_channels == 1
    assert not Cascade(_arch_b()).ensemble
    with pytest.raises(ValueError, match="Cascade takes VisionTransformer"):
        Cascade(Ensemble(_arch_a()))
    with pytest.raises(ValueError, match="3 classes"):
        Cascade(Ensemble(_arch_b(classes=2)))


def test_pinned_tuples():
    from ultrasound_modeling_amd import TBIEvaluator as T
    assert T.PolarResult._fields == ("prob_map", "bleed_prob", "mask", "label", "bmode", "names")
    assert T.CascadeOutput._fields == ("probs", "mask", "prob_map", "bleed_prob")
    assert T.EnsembleCascadeOutput._fields == T.CascadeOutput._fields + ("entropy", "mutual_info", "image_scores")
    assert T.PolarUncertainty._fields == ("result", "entropy", "mutual_info", "image_scores")


def test_python_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    from ultrasound_modeling_amd import ops
    p = torch.zeros(1, 2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ensemble_merge([p])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.calibration_bins(p, p, torch.zeros(47, dtype=torch.int64))
    with pytest.raises(ValueError, match="members"):
        ops.ensemble_merge([])
    with pytest.raises(ValueError, match="members"):
        ops.ensemble_merge([p] * 17)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.ensemble_merge([p.double()])


def test_calibration_from_counts_matches_the_restatement():
    from ultrasound_modeling_amd.metrics import calibration_from_counts, calibration_line
    rng = np.random.default_rng(5)
    probs = _softmax(2 * rng.standard_normal((2, 5, 7, 3)))
    y = np.eye(3, dtype=np.float32)[rng.integers(0, 3, (2, 5, 7))]
    counts, _, _ = R.calibration(probs, y, 15)
    got, want = calibration_from_counts(counts), R.scores_from_counts(counts)
    for k in ("ece", "mce", "brier", "n_invalid"):
        assert got[k] == want[k], k
    for k in ("n", "accuracy", "confidence"):
        assert np.array_equal(got[k], want[k]), k
    assert 0 < got["ece"] < 1 and "ECE" in calibration_line(got)
    empty = calibration_from_counts(np.zeros(5, np.int64))
    assert math.isnan(empty["ece"]) and math.isnan(empty["brier"]) and empty["n"].tolist() == [0]
    with pytest.raises(ValueError):
        calibration_from_counts(np.zeros(6, np.int64))


def test_csv_writers(tmp_path):
    from ultrasound_modeling_amd import TBIEvaluator as T
    p = tmp_path / "u.csv"
    assert T.write_uncertainty_csv(p, ["a", "b"], np.array([[0.5, 0.25, 1.0, 0.0], [1, 2, 3, 4]], np.float32)) == 2
    lines = p.read_text().splitlines()
    assert lines[0] == "name,mean_entropy,mean_mutual_info,max_mutual_info,mean_entropy_bleed" and lines[1] == "a,0.5,0.25,1.0,0.0"
    with pytest.raises(ValueError):
        T.write_uncertainty_csv(p, ["a"], np.zeros((2, 4)))
    counts, _, _ = R.calibration(np.full((1, 1, 2, 2), 0.5, np.float32), np.eye(2, dtype=np.float32).reshape(1, 1, 2, 2), 2)
    q = tmp_path / "c.csv"
    assert T.write_calibration_csv(q, R.scores_from_counts(counts)) == 2
    rows = q.read_text().splitlines()
    assert len(rows) == 4 and rows[2].startswith("1,0.5,1.0,2,0.5,0.5") and rows[3].startswith("total,,,2,,,0.0,0.0,0.5,0")


def test_main_refuses_inconsistent_options_before_it_loads_anything():
    from ultrasound_modeling_amd import TBIEvaluator as T
    base = ["d.npy", "p.npy", "axes", "out", "--bleed", "b.ckpt"]
    for extra in (["--uncertainty-csv", "u.csv"], ["--calibration-csv", "c.csv", "--calibration-bins", "65"], ["--calibration-bins", "0"],
                  ["--tta", "rotate"], ["--tta", "flip"] + ["--bleed-extra", "x.ckpt"] * 8):
        with pytest.raises(SystemExit):
            T.main(base + extra)
