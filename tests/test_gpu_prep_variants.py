"""The two other dataset builders on the GPU (ultrasound_modeling_amd/PizzaPlayGround.py and DataPreprocessing.py, csrc/prep.hip's
usseg_prep_label_thick) against the NumPy restatement of tests/prep_variants_restatement.py: both label orders bit for bit at raw sizes
that upscale one axis and downscale the other, exact 2x ratios and NaN masks; each builder's process_file bit for bit (the B-mode
channel, whose log10 runs on two different libraries, within 1e-12 of the restatement and bit for bit equal to DataFilePlayGround's
output of the same file); both builders end to end on synthetic patient trees; and the pizza set through Dataset_2 and Polar_Model."""
import os

import numpy as np
import pytest
import torch

import prep_restatement as R
import prep_variants_restatement as V

pytestmark = pytest.mark.gpu
DEV = "cuda"

# raw sizes: displacement (H0, W0), B-mode (Hq, Wq, F), bloodMaskThick (Hm, Wm), brain (Hb, Wb); the output is 256 x 80
CASES = {
    "upH_downW": dict(H0=37, W0=123, Hq=300, Wq=41, F=3, Hm=61, Wm=97, Hb=512, Wb=40),
    "exact2x": dict(H0=128, W0=40, Hq=128, Wq=40, F=1, Hm=128, Wm=40, Hb=128, Wb=40),
    "downH_upW": dict(H0=301, W0=17, Hq=33, Wq=161, F=4, Hm=9, Wm=300, Hb=257, Wb=81),
    "down2x": dict(H0=64, W0=64, Hq=64, Wq=64, F=2, Hm=512, Wm=160, Hb=256, Wb=80),
}


def _same(got, ref):
    """Bit for bit, NaN for NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan)
    ints = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(ints)[~nan], ref.view(ints)[~nan])


def _file(tmp_path, case, C=3, seed=0, nan_thick=True):
    from scipy.io import loadmat, savemat
    m = V.make_mat(np.random.default_rng(seed), C=C, nan_thick=nan_thick, zero_channel=True, log_zero=True, **CASES[case])
    path = str(tmp_path / f"DoD008_Ter001_RC2_{case}.mat")
    savemat(path, m)
    return path, loadmat(path)


def _thick(brain, blood, order):
    from ultrasound_modeling_amd import ops
    label, gate = ops.prep_label_thick(torch.from_numpy(np.ascontiguousarray(brain, np.float64)).to(DEV),
                                       torch.from_numpy(np.ascontiguousarray(blood, np.float64)).to(DEV), order)
    return label.cpu().numpy(), gate.cpu().numpy().astype(bool)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_label_thick_kernel(tmp_path, case, order):
    _, mat = _file(tmp_path, case)
    label, gate = _thick(mat["brainMask"], mat["bloodMaskThick"], order)
    ref_label, ref_gate = V.label_thick(mat["brainMask"], mat["bloodMaskThick"], order)
    assert 0 < ref_gate.sum() < ref_gate.size and np.isnan(ref_label).any() and (ref_label > 1).any()
    np.testing.assert_array_equal(gate, ref_gate)
    _same(label, ref_label)
    again, _ = _thick(mat["brainMask"], mat["bloodMaskThick"], order)
    _same(again, label)


def test_label_thick_kernel_known_answers():
    ulp = 2.0 ** -23
    blood = np.tile([0.4 * ulp, 0.8 * ulp], (256, 80))                  # the orders differ in the last bit (test_cpu_prep_variants.py)
    l0, _ = _thick(np.ones((256, 80)), blood, 0)
    l1, _ = _thick(np.ones((256, 80)), blood, 1)
    assert (l0 == np.float32(1)).all() and (l1 == np.float32(1 + ulp)).all()
    hot = np.zeros((128, 40))
    hot[50, 20] = 1.0
    hot[1, 10] = np.nan
    for order in (0, 1):
        label, gate = _thick(np.ones((128, 40)), hot, order)
        assert not gate.any()
        _same(label, V.label_thick(np.ones((128, 40)), hot, order)[0])
        assert np.isnan(label[0:5, 19:23]).all() and np.isnan(label).sum() == 20 and label[100, 40] == np.float32(1.5625)


def _dfp(tmp_path, mat, objective):
    """DataFilePlayGround.process_file of the same displacement, B-mode and brain mask: the channels the builders share with it."""
    from scipy.io import savemat
    from ultrasound_modeling_amd.DataFilePlayGround import process_file
    path = str(tmp_path / "dfp.mat")
    savemat(path, {k: mat[k] for k in ("displacement", "hrTimes", "bModeNorm", "brainMask", "bloodMask", "normalMask")})
    return process_file(path, objective)[0].cpu().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_pizza_process_file(tmp_path, case):
    from ultrasound_modeling_amd.PizzaPlayGround import process_file
    path, mat = _file(tmp_path, case)
    images, name = process_file(path)
    assert name == os.path.basename(path)[:17] and images.is_cuda and images.dtype == torch.float64
    got = images.cpu().numpy()
    ref = V.pizza_file(mat)
    assert got.shape == ref.shape == (3, 1, 256, 80, 12)
    _same(got[..., :11], ref[..., :11])
    assert not np.isfinite(ref[0, ..., 11]).all()
    np.testing.assert_allclose(got[..., 11], ref[..., 11], rtol=0, atol=1e-12, equal_nan=True)
    _same(got[..., 1:], _dfp(tmp_path, mat, 1)[..., 1:])
    assert (got[0, ..., 3] == 0).all()                                  # the all-zero plane normalises to zeros


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_dp_process_file(tmp_path, case, objective):
    from ultrasound_modeling_amd.DataPreprocessing import process_file
    path, mat = _file(tmp_path, case)
    images, name = process_file(path, objective)
    assert name == os.path.basename(path)[:17] + "_cycle2"
    got = images.cpu().numpy()
    ref, k = V.dp_file(mat, objective)
    assert k == 2 and got.shape == ref.shape == (1, 1, 256, 80, 12)
    _same(got[..., :11], ref[..., :11])
    np.testing.assert_allclose(got[..., 11], ref[..., 11], rtol=0, atol=1e-12, equal_nan=True)
    dfp = _dfp(tmp_path, mat, objective)[2:]                            # DataFilePlayGround's last cycle
    _same(got[..., 1:], dfp[..., 1:])
    if objective == 0:
        _same(got, dfp)


def _plan_iteration(raw):
    from ultrasound_modeling_amd.PizzaPlayGround import patient_plan
    for it in range(10):
        plan = patient_plan(it, raw)
        if 0 < sum(t for _, _, t in plan) < len(plan):
            return it, plan
    raise AssertionError("no iteration splits the synthetic tree")


def _compare(got, ref):
    assert got.shape == ref.shape and got.dtype == np.float64
    _same(got[..., :11], ref[..., :11])
    np.testing.assert_allclose(got[..., 11], ref[..., 11], rtol=0, atol=1e-12, equal_nan=True)


def test_pizza_end_to_end(tmp_path):
    from ultrasound_modeling_amd import PizzaPlayGround as P
    patients = (1, 8, 9, 10, 12, 22, 27, 47, 53, 62, 69, 74, 90)
    raw = V.write_tree(str(tmp_path / "raw"), patients, seed=3, empty=((9, 1),), no_cycle=((10, 0),))
    it, plan = _plan_iteration(raw)
    assert {n for n, _, _ in plan} == {"DoD%03d" % p for p in (8, 9, 10, 12, 22, 47, 53, 62, 74)}
    save = str(tmp_path / "pizza_IPH" / "9")
    P.main([raw, save, "--iteration", str(it), "--seed", "4321"])
    assert sorted(os.listdir(save)) == ["axis", "bleed"]
    assert sorted(os.listdir(os.path.join(save, "axis"))) == ["xAxis.npy", "yAxis.npy"]
    d = os.path.join(save, "bleed")
    tr, te = np.load(os.path.join(d, "TrainingData.npy")), np.load(os.path.join(d, "TestingData.npy"))
    trp, tep = np.load(os.path.join(d, "TrainingPaths.npy")), np.load(os.path.join(d, "TestingPaths.npy"))
    r_tr, r_te, r_trp, r_tep = V.pizza_driver(it, raw, 4321)
    assert len(tr) > 0 and len(te) > 0 and trp.shape == (len(tr), 1) and tep.shape == (len(te), 1)
    np.testing.assert_array_equal(trp, r_trp)
    np.testing.assert_array_equal(tep, r_tep)
    _compare(tr, r_tr)
    _compare(te, r_te)
    seen = {p[:17] for p in np.concatenate([trp, tep])[:, 0]}
    assert "DoD009_Ter001_RC0" in seen and not any(p.startswith("DoD009_Ter002") or p.startswith("DoD009_Ter003") for p in seen)
    assert not any(p.startswith("DoD010_Ter001") for p in seen)
    assert not {p[:6] for p in seen} & {"DoD001", "DoD027", "DoD069", "DoD090"}


def test_dp_main_end_to_end(tmp_path):
    from ultrasound_modeling_amd import DataPreprocessing as D
    raw = V.write_tree(str(tmp_path / "raw"), (3, 8, 12, 27, 40), seed=4, empty=((8, 1),), no_cycle=((12, 0),))
    save = str(tmp_path / "out")
    D.main([raw, save, "--seed", "5"])
    assert sorted(os.listdir(save)) == ["axis", "bleed", "brain"]
    for objective, folder in ((0, "brain"), (1, "bleed")):
        d = os.path.join(save, folder)
        tr, te = np.load(os.path.join(d, "TrainingData.npy")), np.load(os.path.join(d, "TestingData.npy"))
        trp, tep = np.load(os.path.join(d, "TrainingPaths.npy")), np.load(os.path.join(d, "TestingPaths.npy"))
        r_tr, r_te, r_trp, r_tep = V.dp_driver(objective, raw)
        assert len(tr) > 0 and len(te) > 0 and trp.shape == (len(tr), 1) and tep.shape == (len(te), 1)
        np.testing.assert_array_equal(trp, r_trp)
        np.testing.assert_array_equal(tep, r_tep)
        _compare(tr, r_tr)
        _compare(te, r_te)
        names = list(np.concatenate([trp, tep])[:, 0])
        assert all("_cycle" in n for n in names) and len(set(names)) == len(names)
        assert {n[:6] for n in tep[:, 0]} | {n[:6] for n in trp[:, 0]} <= {"DoD%03d" % p for p in (3, 8, 12, 27, 40)}
        assert not any(n.startswith("DoD012_Ter001") for n in names)                 # the no-cycle file
        assert not any(n.startswith("DoD008_Ter002") for n in names)                 # after the empty mask
        a = D.build_arrays(objective, raw)
        assert np.array_equal(a[0], tr) and np.array_equal(a[3], tep)


def test_pizza_set_feeds_dataset_and_polar_model(tmp_path):
    from ultrasound_modeling_amd import PizzaPlayGround as P
    from ultrasound_modeling_amd.Dataset_2 import Dataset
    from ultrasound_modeling_amd.TBIEvaluator import Cascade, Polar_Model
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    raw = V.write_tree(str(tmp_path / "raw"), (8, 9, 10, 12, 22, 47), seed=6, cycles=(2, 2))
    it, _ = _plan_iteration(raw)
    P.output2DImages(it, raw, str(tmp_path), seed=7)
    d = str(tmp_path / "bleed")
    ds = Dataset(os.path.join(d, "TrainingData.npy"), os.path.join(d, "TestingData.npy"), num_classes=3)
    assert (ds.height, ds.width, ds.channel) == (256, 80, 10)
    x, y, _ = ds.next_train(batch_size=2)
    assert tuple(x.shape[:3]) == (2, 256, 80) and tuple(y.shape[:3]) == (2, 256, 80)
    test = np.load(os.path.join(d, "TestingData.npy"))[:2]
    names = np.load(os.path.join(d, "TestingPaths.npy"))[:2, 0]
    cascade = Cascade(VisionTransformer(batch_size=2, num_classes=3, seed=1), VisionTransformer(batch_size=2, num_classes=2, seed=2))
    res = Polar_Model(test, cascade, names=names, batch_size=2)
    assert res.prob_map.shape == (len(test), 256, 80) and np.isfinite(res.prob_map).all()
