"""CPU tests of the offline preprocessing (ultrasound_modeling_amd/DataFilePlayGround.py): known answers of the restated cv2 rules
(tests/prep_restatement.py and the host INTER_AREA), the patient order, split and final shuffle against sklearn, the early return on a
folder that holds data, the file checks, and the argument checks of the three prep entry points."""
import os

import numpy as np
import pytest

import prep_restatement as R


# ------------------------------------------------------------------------------------------------ INTER_LINEAR
def test_linear_exact_2x_up_with_clamped_borders():
    out = R.resize_linear(np.array([[0.0, 1.0], [2.0, 3.0]]), (4, 4))
    np.testing.assert_array_equal(out, [[0, .25, .75, 1], [.5, .75, 1.25, 1.5], [1.5, 1.75, 2.25, 2.5], [2, 2.25, 2.75, 3]])


def test_linear_non_integer_up_and_down():
    # 3 -> 5: f = 0.6*(d+0.5) - 0.5 = -0.2 (clamped to 0), 0.4, 1.0, 1.6, 2.2 (single tap S[2])
    out = R.resize_linear(np.array([[0.0, 10.0, 20.0]]), (1, 5))
    np.testing.assert_allclose(out, [[0, 4, 10, 16, 20]], atol=1e-5)
    # 5 -> 2: f = 2.5*(d+0.5) - 0.5 = 0.75, 3.25
    out = R.resize_linear(np.arange(5.0)[None] * 10, (1, 2))
    np.testing.assert_array_equal(out, [[7.5, 32.5]])
    # 4 -> 2 (exactly 2x down): the mean of each pair
    np.testing.assert_array_equal(R.resize_linear(np.array([[0.0, 1.0, 2.0, 3.0]]), (1, 2)), [[0.5, 2.5]])
    # vertical as horizontal, float32 stays float32, channels are independent
    src = np.stack([np.array([[0.0], [1.0]]), np.array([[2.0], [3.0]])], axis=-1).astype(np.float32)
    out = R.resize_linear(src, (4, 1))
    assert out.dtype == np.float32 and out.shape == (4, 1, 2)
    np.testing.assert_array_equal(out[:, 0, 0], [0, .25, .75, 1])
    np.testing.assert_array_equal(out[:, 0, 1], [2, 2.25, 2.75, 3])


def test_linear_identity_size_and_single_source_pixel():
    x = np.random.default_rng(0).standard_normal((7, 5))
    np.testing.assert_array_equal(R.resize_linear(x, (7, 5)), x)
    np.testing.assert_array_equal(R.resize_linear(np.full((1, 1), 3.5), (3, 2)), np.full((3, 2), 3.5))


# ------------------------------------------------------------------------------------------------ GaussianBlur
def test_gaussian_kernels_and_reflect101():
    for k, s in ((9, 4.0), (3, 2.0)):
        w = R.gauss_kernel(k, s)
        assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6
        np.testing.assert_array_equal(w, w[::-1])
        x = np.arange(k) - (k - 1) / 2
        t = np.exp(-x * x / (2 * s * s))
        np.testing.assert_allclose(w, t / t.sum(), rtol=1e-6)
    np.testing.assert_array_equal(R.reflect101(np.arange(-3, 8), 5), [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1])      # dcb|abcd|cba
    np.testing.assert_array_equal(R.reflect101(np.arange(-2, 3), 1), [0] * 5)


def test_gaussian_blur_impulse_at_the_corner():
    w = R.gauss_kernel(3, 2.0)
    img = np.zeros((5, 5), np.float32)
    img[0, 0] = 1
    out = R.gaussian_blur(img, 3, 2.0)
    # REFLECT_101: the corner's neighbours at -1 reflect to 1, so only the centre tap of each pass sees the impulse at (0, 0)
    np.testing.assert_allclose(out[:2, :2], [[w[1] * w[1], w[1] * w[0]], [w[0] * w[1], w[0] * w[0]]], rtol=1e-7)
    assert out[2:].max() == 0 and out[:, 2:].max() == 0
    const = np.full((6, 4), 2.0, np.float32)
    np.testing.assert_allclose(R.gaussian_blur(const, 9, 4.0), const, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ INTER_AREA (host)
def test_area_box_and_upscale():
    from ultrasound_modeling_amd.DataFilePlayGround import resize_area
    np.testing.assert_allclose(resize_area(np.arange(16.0).reshape(4, 4), (2, 2)), [[2.5, 4.5], [10.5, 12.5]], rtol=1e-7)
    # 5 -> 2: cells of 2.5 source pixels: weights 0.4, 0.4, 0.2 | 0.2, 0.4, 0.4
    np.testing.assert_allclose(resize_area(np.arange(5.0)[None], (1, 2)), [[0.8, 3.2]], rtol=1e-6)
    # 2 -> 4 on both axes (growing): the area coefficients pick the nearest source pixel
    np.testing.assert_array_equal(resize_area(np.array([[0.0, 1.0], [2.0, 3.0]]), (4, 4)),
                                  [[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [2, 2, 3, 3]])
    # one axis grows (4 -> 8), the other shrinks (6 -> 3): the linear scheme with area coefficients on both axes
    src = np.arange(24.0).reshape(4, 6)
    out = resize_area(src, (8, 3))
    assert out.shape == (8, 3)
    # rows: f = (d+1) - (s+1)*2 <= 0 everywhere (nearest row); columns: f = (d+1) - (2d+1)/2 = 0.5 (the mean of a pair)
    np.testing.assert_array_equal(out, np.repeat((src[:, 0::2] + src[:, 1::2]) / 2, 2, axis=0))
    np.testing.assert_allclose(resize_area(np.full((300, 120), 7.0)), np.full((256, 80), 7.0), rtol=1e-6)


def test_fetch_polar_axis(tmp_path):
    from scipy.io import savemat
    from ultrasound_modeling_amd.DataFilePlayGround import FetchPolarAxis, resize_area
    m = R.make_mat(np.random.default_rng(3), H0=300, W0=100, axis=True)
    savemat(str(tmp_path / "f.mat"), m)
    FetchPolarAxis(str(tmp_path / "f.mat"), str(tmp_path))
    x, y = np.load(tmp_path / "xAxis.npy"), np.load(tmp_path / "yAxis.npy")
    assert x.shape == y.shape == (256, 80)
    np.testing.assert_allclose(x, resize_area(m["xAxis"]) + 100)
    np.testing.assert_allclose(y, resize_area(m["zAxis"]) - 4)


# ------------------------------------------------------------------------------------------------ order, split, shuffle
def _folders(root, n, extra=()):
    for p in list(range(1, n + 1)) + list(extra):
        os.makedirs(os.path.join(root, "DoD%03d" % p))
    return str(root)


def test_patient_order_is_sklearn_shuffle(tmp_path):
    shuffle = pytest.importorskip("sklearn.utils").shuffle
    from ultrasound_modeling_amd.DataFilePlayGround import patient_plan, permutation
    raw = _folders(tmp_path, 40, extra=(928,))
    expected = shuffle(np.sort(os.listdir(raw)), random_state=20)
    plan = patient_plan(1, raw)
    for name, index, _ in plan:
        assert expected[index] == name
    for n, seed in ((0, 3), (1, 5), (17, 0), (50, 99999), (50, 99999 // 17)):
        rows = np.arange(n * 3).reshape(n, 3)
        np.testing.assert_array_equal(rows[permutation(n, seed)], shuffle(rows, random_state=seed))


def test_split_by_patient_index_counts_bad_patients(tmp_path):
    from ultrasound_modeling_amd.DataFilePlayGround import BAD_PATIENTS, patient_plan
    raw = _folders(tmp_path, 30)
    names = np.sort(os.listdir(raw))[np.random.RandomState(20).permutation(30)]
    for iteration in (1, 4, 13):
        plan = patient_plan(iteration, raw)
        assert [p[0] for p in plan] == [n for n in names if int(n[-3:]) not in BAD_PATIENTS]
        for name, index, is_test in plan:
            assert names[index] == name                                   # skipped patients keep their place in the count
            assert is_test == (index % 10 == iteration % 10)
        assert {p[0] for p in plan}.isdisjoint({"DoD%03d" % b for b in BAD_PATIENTS})
    assert len(patient_plan(1, raw)) == 30 - sum(1 for b in BAD_PATIENTS if b <= 30)


def test_early_return_on_a_folder_with_data(tmp_path, capsys):
    from ultrasound_modeling_amd.DataFilePlayGround import output2DImages
    for obj, folder in ((0, "brainMask"), (1, "bleed")):
        d = tmp_path / folder
        d.mkdir()
        (d / "keep.txt").write_text("x")
        assert output2DImages(1, obj, str(tmp_path / "no_such_raw_folder"), str(tmp_path)) is None
        assert os.listdir(d) == ["keep.txt"]
        assert "contains data" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ malformed files
@pytest.mark.parametrize("case", ["past_end", "negative_start", "bmode_3d", "bmode_short", "missing", "masks_differ"])
def test_malformed_file_raises_naming_it(tmp_path, case):
    from scipy.io import savemat
    from ultrasound_modeling_amd.DataFilePlayGround import process_file
    m = R.make_mat(np.random.default_rng(1), C=3)
    if case == "past_end":
        m["displacement"] = m["displacement"][:, :, :-5]
    elif case == "negative_start":
        m["hrTimes"] = m["hrTimes"] - 1.0
    elif case == "bmode_3d":
        m["bModeNorm"] = m["bModeNorm"][:, :, :, 0]
    elif case == "bmode_short":
        m["bModeNorm"] = m["bModeNorm"][:, :, :, :2]
    elif case == "missing":
        del m["hrTimes"]
    else:
        m["normalMask"] = m["normalMask"][:-1]
    path = str(tmp_path / ("DoD005_%s.mat" % case))
    savemat(path, m)
    for objective in (0, 1):
        with pytest.raises(ValueError, match="DoD005_" + case):
            process_file(path, objective, device="cpu")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_prep_entry_points_reject_bad_arguments():
    from ultrasound_modeling_amd import _lib
    lib = _lib.load()
    assert lib.usseg_prep_cycle_stats(16, 0, 8, 8, 16, 16, None) == -1 and b"geometry" in lib.usseg_last_error()
    assert lib.usseg_prep_cycle_stats(None, 1, 8, 8, 16, 16, None) == -1 and b"null pointer" in lib.usseg_last_error()
    assert lib.usseg_prep_label(16, 8, 8, None, None, 0, 0, 2, None, 16, 16, None) == -1 and b"objective" in lib.usseg_last_error()
    assert lib.usseg_prep_label(16, 8, 8, None, None, 8, 8, 1, None, 16, 16, None) == -1 and b"objective 1 needs" in lib.usseg_last_error()
    assert lib.usseg_prep_label(16, 0, 8, None, None, 0, 0, 0, None, 16, 16, None) == -1 and b"brain-mask" in lib.usseg_last_error()
    assert lib.usseg_prep_assemble(16, 16, 2, 8, 8, 16, 8, 8, 0, 16, 16, 0, 16, None) == -1 and b"B-mode" in lib.usseg_last_error()
    assert lib.usseg_prep_assemble(16, 16, 2, 8, 8, 16, 8, 8, 3, 16, None, 0, 16, None) == -1 and b"null pointer" in lib.usseg_last_error()
