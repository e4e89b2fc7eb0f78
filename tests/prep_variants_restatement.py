"""A NumPy restatement of the two other dataset builders of the reference - PizzaPlayGround.output2DImages (the IPH-only "pizza" bleed set)
and DataPreprocessing.py - written from the reference's scripts and the cv2 rules of tests/prep_restatement.py, not from the kernels, plus
a writer of small synthetic raw trees that carry bloodMaskThick.

Labels (no blur, no normalMask):
  order 0 (PizzaPlayGround.py:92-97): cv2.resize(float32(bloodMaskThick + 1)) in float32, 0 where the resized brain mask is 0;
  order 1 (DataPreprocessing.py:134-146): float32(cv2.resize(bloodMaskThick) + 1) with the fp64 resize, 0 where the brain mask is 0.
"""
import math
import os

import numpy as np

import prep_restatement as R

F32, F64 = np.float32, np.float64
H_OUT, W_OUT = R.H_OUT, R.W_OUT
IPH = (8, 9, 10, 12, 22, 47, 53, 62, 66, 67, 69, 74, 75, 78, 85, 89, 93, 101, 105, 107, 110, 112, 113, 120, 121, 126, 129, 130, 133)
PIZZA_BAD = (27, 28, 35, 36, 38, 49, 69, 90)


def label_thick(brain, blood, order):
    """-> (label float32 [256,80], gate bool [256,80])."""
    gate = R.resize_linear(np.asarray(brain, F64)) == 0
    blood = np.asarray(blood, F64)
    with np.errstate(invalid="ignore"):
        if order == 0:
            lab = R.resize_linear((blood + 1).astype(F32))
        else:
            lab = (R.resize_linear(blood) + 1).astype(F32)
    return np.where(gate, F32(0), lab).astype(F32), gate


def _mask_label(brain):
    gate = R.resize_linear(np.asarray(brain, F64)) == 0
    return np.where(gate, 0, 1).astype(F32), gate


def _cycle_planes(disp, hr, width):
    """The reference's C-order gather of every cycle's frames: ``width`` = 10 gives DataPreprocessing's displace_data [H,W,10,C]
    (:56-59), 5 PizzaPlayGround's real and imag [H,W,5,C] (:80-85).  The layout fixes numpy's summation order in the means (a sum over
    the outer axis 0 adds row after row), which is the order the kernels use."""
    C = hr.shape[1] - 1
    out = [np.zeros(disp.shape[:2] + (width, C)) for _ in range(10 // width)]
    for h in range(C):
        start = int(math.ceil(30 * hr[0, h]))
        for i, o in enumerate(out):
            o[:, :, :, h] = disp[:, :, start + i * width:start + (i + 1) * width]
    return out


def _image(planes, bmode, h, label, gate, gated):
    frames = np.concatenate([R.resize_linear(R.normalise(p[:, :, :, h])) for p in planes], axis=2)
    if gated:
        frames[gate] = 0.0
    with np.errstate(invalid="ignore"):
        b = R.resize_linear(np.ascontiguousarray(bmode[:, :, h]))
    return np.concatenate([label[..., None].astype(F64), frames, b[..., None]], axis=2)[None]


def _fields(mat):
    """displacement, hrTimes and mean_F log10(bModeNorm), C-ordered as the reference's np.array(list(mat[k])) makes them."""
    disp = np.ascontiguousarray(mat["displacement"], F64)
    hr = np.asarray(mat["hrTimes"], F64)
    with np.errstate(divide="ignore"):
        bmode = np.log10(np.ascontiguousarray(mat["bModeNorm"], F64)).mean(axis=2)
    return disp, hr, bmode


def pizza_file(mat):
    """One loaded file -> float64 [C,1,256,80,12], every cycle (PizzaPlayGround.py:59-145), or None for an empty bloodMaskThick."""
    if len(np.asarray(mat["bloodMaskThick"])) == 0:
        return None
    disp, hr, bmode = _fields(mat)
    label, gate = label_thick(mat["brainMask"], mat["bloodMaskThick"], 0)
    planes = _cycle_planes(disp, hr, 5)
    out = [_image(planes, bmode, h, label, gate, True) for h in range(hr.shape[1] - 1)]
    return np.array(out).reshape(-1, 1, H_OUT, W_OUT, 12)


def dp_file(mat, objective):
    """One loaded file -> (float64 [n,1,256,80,12], cycle index) with n = 1 (the last cycle, DataPreprocessing.py:129-169) or 0 (no
    cycle), or None for an empty bloodMaskThick."""
    if len(np.asarray(mat["bloodMaskThick"])) == 0:
        return None
    disp, hr, bmode = _fields(mat)
    C = hr.shape[1] - 1
    if C == 0:
        return np.zeros((0, 1, H_OUT, W_OUT, 12)), None
    label, gate = _mask_label(mat["brainMask"]) if objective == 0 else label_thick(mat["brainMask"], mat["bloodMaskThick"], 1)
    return _image(_cycle_planes(disp, hr, 10), bmode, C - 1, label, gate, objective == 1)[None], C - 1


def pizza_driver(iteration, raw, seed):
    """PizzaPlayGround.output2DImages in one process (sorted files) -> (train, test, train_paths, test_paths)."""
    from scipy.io import loadmat
    names = np.sort(os.listdir(raw))
    names = names[np.random.RandomState(20).permutation(len(names))]
    tr, te, trp, tep = [], [], [], []
    for count, name in enumerate(names):
        num = int(name[-3:])
        if num in PIZZA_BAD or num not in IPH:
            continue
        for f in sorted(os.listdir(os.path.join(raw, name))):
            if ".mat" not in f:
                continue
            imgs = pizza_file(loadmat(os.path.join(raw, name, f)))
            if imgs is None:
                break
            for img in imgs:
                if count % 10 == iteration % 10:
                    te.append(img), tep.append([f[0:17]])
                else:
                    tr.append(img), trp.append([f[0:17]])

    def shuf(rows, paths, s):
        p = np.random.RandomState(s).permutation(len(rows))
        data = np.array(rows).reshape(-1, 1, H_OUT, W_OUT, 12)[p]
        return data, np.array(paths, dtype=str).reshape(-1, 1)[p]
    train, train_paths = shuf(tr, trp, seed)
    test, test_paths = shuf(te, tep, seed // 17)
    return train, test, train_paths, test_paths


def dp_split(P, test_size=0.5, seed=42):
    """train_test_split's patient indices: (train, test)."""
    n_test = math.ceil(test_size * P)
    perm = np.random.RandomState(seed).permutation(P)
    return perm[n_test:], perm[:n_test]


def dp_driver(objective, raw):
    """DataPreprocessing's process_patients + split_data(test_size=0.5) over sorted patients and files -> (train, test, train_paths,
    test_paths) with rows [N,1,256,80,12] and paths [N,1]."""
    from scipy.io import loadmat
    per_rows, per_names = [], []
    for name in sorted(os.listdir(raw)):
        rows, names = [], []
        for f in sorted(os.listdir(os.path.join(raw, name))):
            if ".mat" not in f:
                continue
            res = dp_file(loadmat(os.path.join(raw, name, f)), objective)
            if res is None:
                break
            imgs, k = res
            if len(imgs):
                rows.append(imgs[0])
                names.append(f[0:17] + "_cycle" + str(k))
        per_rows.append(rows)
        per_names.append(names)
    train_idx, test_idx = dp_split(len(per_rows))

    def side(idx):
        rows = [r for i in idx for r in per_rows[i]]
        data = np.array(rows).reshape(-1, 1, H_OUT, W_OUT, 12)
        return data, np.array([n for i in idx for n in per_names[i]], dtype=str).reshape(-1, 1)
    train, train_paths = side(train_idx)
    test, test_paths = side(test_idx)
    return train, test, train_paths, test_paths


# ------------------------------------------------------------------------------------------------ synthetic raw data
def make_mat(rng, nan_thick=False, **kw):
    """R.make_mat's dict plus bloodMaskThick (the blood mask's size): a thick 0/1 region with a soft edge, NaNs if nan_thick."""
    m = R.make_mat(rng, nan_blood=nan_thick, **kw)
    Hm, Wm = m["bloodMask"].shape
    yy, xx = np.mgrid[0:Hm, 0:Wm]
    thick = np.clip(1.5 - np.hypot((yy - Hm / 2.5) / (0.2 * Hm), (xx - Wm / 2) / (0.25 * Wm)), 0, 1) * rng.uniform(0.9, 1.0)
    if nan_thick:
        thick[rng.uniform(size=(Hm, Wm)) < 0.05] = np.nan
    m["bloodMaskThick"] = thick
    return m


def write_tree(root, patients, seed=0, files=(1, 2), cycles=(1, 3), size=(37, 23), empty=(), no_cycle=()):
    """Patient folders DoD<nnn> for each number in ``patients`` with 1-2 .mat files each; ``empty`` names (patient, file index) whose
    bloodMaskThick is empty, ``no_cycle`` those whose hrTimes holds no cycle.  Returns the root."""
    from scipy.io import savemat
    rng = np.random.default_rng(seed)
    for p in patients:
        d = os.path.join(root, "DoD%03d" % p)
        os.makedirs(d)
        nf = int(rng.integers(files[0], files[1] + 1))
        for f in range(max(nf, max([i + 1 for q, i in empty + no_cycle if q == p], default=0))):
            m = make_mat(rng, H0=size[0], W0=size[1], C=int(rng.integers(cycles[0], cycles[1] + 1)), axis=True)
            if (p, f) in empty:
                m["bloodMaskThick"] = np.zeros((0, 0))
            if (p, f) in no_cycle:
                m["hrTimes"] = m["hrTimes"][:, :1]
            savemat(os.path.join(d, "DoD%03d_Ter%03d_RC%d_Displacement_Polar.mat" % (p, f + 1, p % 3)), m)
    return root
