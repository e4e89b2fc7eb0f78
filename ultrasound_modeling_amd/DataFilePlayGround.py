"""The reference's offline data preparation ``DataFilePlayGround.output2DImages`` (DataFilePlayGround.py:249-515): a patient's raw ``.mat``
scans -> the ``TrainingData.npy`` / ``TestingData.npy`` [N,1,256,80,12] arrays and their paths that ``Dataset_2``, ``MainNumpy``,
``MainParallel`` and ``TBIEvaluator`` read.  Channel 0 is the label, 1-10 the normalised displacement frames of one cardiac cycle, 11 the
B-mode image.  Folders ``brainMask/`` (objective 0) and ``bleed/`` (objective 1) as in the reference.

The numeric work of a file runs on the device, every cycle of the file at once (csrc/prep.hip): ``process_file`` gathers the 10*C frames
the file's cycles use into one buffer with the B-mode stack and the masks, makes one host-to-device copy and enqueues three short steps on
the current stream - per-plane statistics, the label and gate, and the assembly of the 12 channels - with no host synchronisation.  The
host keeps ``loadmat``, the file walk, the split and the saves.

cv2 is not part of this stack.  The kernels and ``resize_area`` restate the cv2 functions the reference calls, from these rules (a
restatement of cv2's documented behaviour, not checked against cv2 itself):
  * ``resize`` INTER_LINEAR, per axis: ``inv = dsize/ssize``, ``scale = 1.0/inv`` (double); ``f = float32((d+0.5)*scale - 0.5)``,
    ``s = floor(f)``, ``f -= s`` (float32).  ``s < 0`` -> ``s, f = 0, 0``; ``s >= ssize-1`` -> ``s, f = ssize-1, 0`` and only the single
    horizontal tap ``S[s]`` is used.  Weights float32 ``(1-f, f)``.  The horizontal pass first, then the vertical
    ``b0*row(s) + b1*row(min(s+1, ssize-1))``.  float64 input: the weights are applied in double; float32 input: all in float32.
  * ``GaussianBlur(ksize, sigma)`` on float32: ``t_i = float32(exp(-x_i^2/(2 sigma^2)))``, ``w_i = float32(t_i * (1/sum t))``;
    separable, rows then columns, border BORDER_REFLECT_101 (``dcb|abcd|cba``).
  * ``resize`` INTER_AREA (``FetchPolarAxis`` only, host NumPy): box averages when neither axis grows, else the linear scheme with the
    area coefficients ``s = floor(d*scale)``, ``f = (d+1) - (s+1)*inv``, ``f = 0 if f <= 0 else f - floor(f)``.

Deliberate deviations from the reference:
  * one process: patients in the shuffled order, the ``.mat`` files of a patient in sorted order (the reference forks one child per
    patient and appends in whatever order the children finish, and walks a patient's files in ``os.listdir`` order);
  * ``seed=None`` draws the final shuffle's seed as the reference does (``np.random.randint(0, 1e5)``); a given ``seed`` reproduces the
    output exactly;
  * every input array is converted to float64 first, integer and boolean masks included (cv2's 8-bit fixed-point resize is not
    restated; the reference's masks carry NaNs, so they are floating point), and ``log10`` is taken in float64;
  * a file that lacks a field, has a cycle window that starts before frame 0 or runs past the last frame, or whose ``bModeNorm`` is not
    4-D with a slice per cycle raises a ``ValueError`` naming the file (the reference fails inside a child process or mis-slices);
  * the output folder's parent is created if it is missing.

``dataAug`` (:177-246) and the oversampling block written for it (:404-433, commented out in the reference: "my server does not have the RAM
required to run it") run on the device too (csrc/prep_aug.hip, seven launches per batch whatever the draws are); DESIGN.md section 4h
defines every step as the reference EXECUTES it.  The draws stay on the host in the reference's order (``draw_aug``).  Deviations:
  * contrast: where the reference would divide by zero (the stretched channels are constant, or the 2nd and 98th percentile coincide)
    the contrast step is skipped for that sample;
  * noise: the reference draws its Gaussian from NumPy's global generator; here a counter-based generator on the device, seeded per
    sample from the draws, or a field given by the caller;
  * oversampling: the original row is kept unchanged and every copy starts from the original (the block's ``imageA = image`` is an alias:
    it would chain the augmentations and overwrite the original); the bleed fraction divides by H*W and counts label pixels >= 1.05,
    ``label2vec``'s class-2 threshold (the commented line :350 divides ``label == 2`` counts by a stale 256*64).
Records are expected to be finite: a NaN or an infinity makes the contrast step's minimum, maximum and percentiles meaningless.
"""
from __future__ import annotations

import argparse
import math
import os
import ctypes as C
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops

OUT_H, OUT_W = ops.PREP_H, ops.PREP_W
PATIENT_SEED = 20          # sklearn.utils.shuffle(pathlist, random_state=20), :444
BAD_PATIENTS = (1, 14, 22, 23, 27, 28, 32, 34, 35, 36, 37, 38, 39, 44, 49, 69, 71, 78, 82, 90, 98, 101, 121, 124, 128, 133, 136, 928)  # :278
IPH_PATIENTS = (8, 9, 10, 12, 22, 47, 53, 62, 66, 67, 69, 74, 75, 78, 85, 89, 93, 101, 105, 107, 110, 112, 113, 120, 121, 126, 129, 130, 133)  # :276-277
OVERSAMPLE_MODES = (None, "bleed", "all")
FIELDS = ("normalMask", "bloodMask", "brainMask", "bModeNorm", "displacement", "hrTimes")


def permutation(n: int, seed: int) -> np.ndarray:
    """The order ``sklearn.utils.shuffle(x, random_state=seed)`` puts n rows in: ``np.random.RandomState(seed).permutation(n)``."""
    return np.random.RandomState(seed).permutation(n)


def patient_plan(iteration: int, rawDataPath: str) -> List[Tuple[str, int, bool]]:
    """The patients ``output2DImages`` processes, in its order: (folder name, index in the shuffled list, goes to the test set).
    The list is every entry of ``rawDataPath``, sorted, then shuffled with random_state 20 (:442-444); a bad patient (:278-279,
    ``int(name[-3:])``) is left out but keeps its index; a patient is a test patient iff index % 10 == iteration % 10 (:397)."""
    names = np.sort(os.listdir(rawDataPath))
    names = names[permutation(len(names), PATIENT_SEED)]
    plan = []
    for index, name in enumerate(names):
        if int(name[-3:]) in BAD_PATIENTS:
            continue
        plan.append((str(name), index, index % 10 == iteration % 10))
    return plan


def _require(path: str, mat, fields) -> None:
    missing = [k for k in fields if k not in mat]
    if missing:
        raise ValueError(f"{path}: missing {', '.join(missing)}")


def _check(path: str, mat, masks):
    """The shape checks of a loaded file; -> float64 (displacement, hrTimes, bModeNorm, [the fields named by masks])."""
    f64 = lambda k: np.asarray(mat[k]).astype(np.float64)
    disp, hr, bmode = f64("displacement"), f64("hrTimes"), f64("bModeNorm")
    ms = [f64(k) for k in masks]
    if disp.ndim != 3:
        raise ValueError(f"{path}: displacement must be [H, W, T], is {disp.shape}")
    if hr.ndim != 2 or hr.shape[0] < 1 or hr.shape[1] < 1:
        raise ValueError(f"{path}: hrTimes must be [1, cycles + 1], is {hr.shape}")
    C = hr.shape[1] - 1
    if bmode.ndim != 4 or bmode.shape[3] < C or 0 in bmode.shape[:3]:
        raise ValueError(f"{path}: bModeNorm must be [H, W, F, >= {C}], is {bmode.shape}")
    for k, m in zip(masks, ms):
        if m.ndim != 2 or 0 in m.shape:
            raise ValueError(f"{path}: {k} must be a non-empty 2-D array, is {m.shape}")
    return disp, hr, bmode, ms


def _gather(path: str, disp, hr, bmode):
    """-> host float64 (frames [C,10,H0,W0], bmode [C,Hq,Wq,F]): the 10 frames each cycle's window takes (:316) and its B-mode slice."""
    C, T = hr.shape[1] - 1, disp.shape[2]
    frames = np.empty((C, 10) + disp.shape[:2], np.float64)
    for h in range(C):
        start = int(math.ceil(30 * hr[0, h]))          # :316
        if start < 0 or start + 10 > T:
            raise ValueError(f"{path}: cycle {h} takes frames {start}..{start + 9}, the file has {T}")
        frames[h] = np.moveaxis(disp[:, :, start:start + 10], 2, 0)
    return frames, np.ascontiguousarray(np.moveaxis(bmode[:, :, :, :C], 3, 0))


def _load(path: str):
    """Read and check one file; -> host float64 (frames [C,10,H0,W0], bmode [C,Hq,Wq,F], brain, blood, normal)."""
    from scipy.io import loadmat
    mat = loadmat(path)
    _require(path, mat, FIELDS)
    disp, hr, bmode, (brain, blood, normal) = _check(path, mat, ("brainMask", "bloodMask", "normalMask"))
    if blood.shape != normal.shape:
        raise ValueError(f"{path}: bloodMask {blood.shape} and normalMask {normal.shape} differ in shape")
    return _gather(path, disp, hr, bmode) + (brain, blood, normal)


def _upload(parts, device):
    """One host-to-device copy of the host float64 arrays ``parts``; -> a device view of each."""
    dev = torch.from_numpy(np.concatenate([p.ravel() for p in parts])).to(device)
    views, off = [], 0
    for p in parts:
        views.append(dev[off:off + p.size].view(p.shape))
        off += p.size
    return views


def process_file(path: str, objective: int, device="cuda") -> Tuple[torch.Tensor, str]:
    """One ``.mat`` file -> (images, name): images a device float64 [C,1,256,80,12], one per cardiac cycle, as the reference's inner
    loop builds them (:294-393, mode 1); name = the file name's first 17 characters (:291).  Enqueued on the current stream."""
    if objective not in (0, 1):
        raise ValueError(f"objective must be 0 (brain mask) or 1 (bleed), got {objective}")
    frames, bmode, brain, blood, normal = _load(path)
    name = os.path.basename(path)[0:17]
    device = torch.device(device)
    C = frames.shape[0]
    if C == 0:
        return torch.empty((0, 1, OUT_H, OUT_W, 12), dtype=torch.float64, device=device), name
    parts = [frames, bmode, brain] + ([blood, normal] if objective == 1 else [])
    views = _upload(parts, device)                                                         # the one host-to-device copy
    frames_d, bmode_d, brain_d = views[:3]
    stats = ops.prep_cycle_stats(frames_d)
    label, gate = ops.prep_label(brain_d, objective, *views[3:])
    return ops.prep_assemble(frames_d, stats, bmode_d, label, gate, objective), name


# ---------------------------------------------------------------------------------------------------------- dataAug on the device
def draw_aug(rng=random) -> dict:
    """The draws of one ``dataAug`` call (:178-179, :121-124, :104-106), in the reference's order: r, t, the clip box if r % 5, the shift
    if t % 2.  -> the steps the sample takes: flip (r % 2), reduc (r % 3), contrast (t % 3), clip (r, c, ra, ca) or None, rotate (r % 13)
    by angle (r % 11) / 5 degrees, shift (r, c, direction) or None, noise (t % 5) and the seed of the generated noise."""
    r = rng.randint(0, 100000)
    t = rng.randint(0, 100000)
    p = {"r": r, "t": t, "flip": bool(r % 2), "reduc": bool(r % 3), "contrast": bool(t % 3), "clip": None, "rotate": bool(r % 13),
         "angle": (r % 11) / 5, "shift": None, "noise": bool(t % 5), "seed": r * 100003 + t}
    if r % 5:
        p["clip"] = (rng.randint(0, 256), rng.randint(0, 80), rng.randint(20, 40), rng.randint(10, 20))
    if t % 2:
        p["shift"] = (rng.randint(0, 30), rng.randint(0, 12), rng.randint(0, 1))
    return p


REDUC_ONLY = {"flip": False, "reduc": True, "contrast": False, "clip": None, "rotate": False, "angle": 0.0, "shift": None, "noise": False,
              "seed": 0}


def rotation(angle: float, H: int, W: int):
    """The six doubles of ``scipy.ndimage.rotate(image, angle, reshape=False)`` on an [H, W] plane: (R00, R01, R10, R11, offset0, offset1),
    source (y, x) = R (i, j) + offset with R = [[c, s], [-s, c]] and offset = (shape-1)/2 - R (shape-1)/2."""
    from scipy import special
    c, s = np.float64(special.cosdg(angle)), np.float64(special.sindg(angle))
    R = np.array([[c, s], [-s, c]], np.float64)
    centre = (np.array([H, W], np.float64) - 1) / 2
    off = centre - R @ centre
    return (float(R[0, 0]), float(R[0, 1]), float(R[1, 0]), float(R[1, 1]), float(off[0]), float(off[1]))


def percentile_position(n: int, q: float) -> Tuple[int, float]:
    """numpy's linear rule: the q-th percentile of n values lies at pos = q/100 * (n-1); -> (floor(pos), pos - floor(pos))."""
    pos = (n - 1) * (q / 100)
    k = int(math.floor(pos))
    return k, pos - k


def _aug_tables(params: List[dict], H: int, W: int, device):
    """-> (table uint8, rot_list int32, n_rot): the N UssegPrepAugSample and the index list of the samples that rotate, one upload."""
    arr = (L.PrepAugSample * len(params))()
    rot = []
    for i, p in enumerate(params):
        s = arr[i]
        s.do_flip, s.do_reduc, s.do_contrast, s.do_noise = int(p["flip"]), int(p["reduc"]), int(p["contrast"]), int(p["noise"])
        if p["clip"] is not None:
            s.do_clip = 1
            for q in range(4):
                s.clip[q] = int(p["clip"][q])
        if p["shift"] is not None:
            s.do_shift, (s.shift_r, s.shift_c, s.shift_dir) = 1, (int(v) for v in p["shift"])
        s.rot_slot = -1
        if p["rotate"]:
            s.do_rotate, s.rot_slot = 1, len(rot)
            rot.append(i)
            for q, v in enumerate(rotation(p["angle"], H, W)):
                s.rot[q] = v
        s.seed = int(p.get("seed", 0)) & ((1 << 63) - 1)
    raw = bytes(arr) + np.asarray(rot or [0], np.int32).tobytes()
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    size = C.sizeof(L.PrepAugSample) * len(params)
    return buf[:size], buf[size:].view(torch.int32), len(rot)


def dataAug_batch(images: torch.Tensor, params: Optional[List[dict]] = None, noise: Optional[torch.Tensor] = None, rng=random, *,
                  noise_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dataAug`` (:177-246) of every record of ``images``, a device float64 [N, H, W, Cc] (Cc >= 3, H, W >= 4; channel 0 the label,
    Cc-1 the B-mode image) -> a new tensor of the same shape; the input is not modified.  ``params``: one ``draw_aug`` dict per record
    (drawn from ``rng`` in order if None).  ``noise``: the unit Gaussian field [N, H, W, Cc-1] to use instead of the device's generator;
    ``noise_out`` (same shape) receives the field that was used.  The contrast step is skipped for a sample whose stretched channels are
    constant or whose 2nd and 98th percentile coincide (the reference divides by zero there)."""
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float64 and images.dim() == 4):
        raise ValueError("dataAug_batch: images must be a float64 cuda tensor [N, H, W, Cc]")
    N, H, W, Cc = images.shape
    if N < 1 or H < 4 or W < 4 or Cc < 3:
        raise ValueError(f"dataAug_batch: need N >= 1, H >= 4, W >= 4, Cc >= 3, got {tuple(images.shape)}")
    if params is None:
        params = [draw_aug(rng) for _ in range(N)]
    if len(params) != N:
        raise ValueError(f"dataAug_batch: {len(params)} parameter sets for {N} records")
    table, rot_list, n_rot = _aug_tables(params, H, W, images.device)
    (k_lo, g_lo), (k_hi, g_hi) = percentile_position(H * W * Cc, 2), percentile_position(H * W * Cc, 98)
    z = math.sqrt(3.0) - 2.0
    return ops.prep_aug(images.contiguous(), table, rot_list, n_rot, k_lo, g_lo, k_hi, g_hi, math.pow(z, H - 1), math.pow(z, W - 1),
                        noise=noise, noise_out=noise_out)


def dataAug(image: torch.Tensor) -> torch.Tensor:
    """The reference's signature (:177): one record [H, W, Cc] on the device -> its augmented copy, the draws from ``random``."""
    return dataAug_batch(image[None])[0]


# ---------------------------------------------------------------------------------------------------------- the oversampling block
def oversample_plan(name: str, patient: int, f: float, mode) -> List[Tuple[str, str]]:
    """The rows appended after a TRAINING record ``name`` of patient number ``patient`` and bleed fraction ``f`` (:404-433):
    [(row name, "reduc" | "aug")].  An IPH patient: name + "iph_0", "iph_1", each imageReduc alone of the original; f > 0.05:
    floor(f / 0.03) rows name + "_0", "_1", ..., each a fresh dataAug of the original; mode "all": name + "aug_0", "aug_1", likewise."""
    if mode not in OVERSAMPLE_MODES:
        raise ValueError(f"oversample must be one of {OVERSAMPLE_MODES}, got {mode!r}")
    rows = []
    if mode is None:
        return rows
    if patient in IPH_PATIENTS:
        rows += [(name + "iph_{}".format(x), "reduc") for x in range(2)]
    if f > 0.05:
        rows += [(name + "_{}".format(y), "aug") for y in range(math.floor(f / 0.03))]
    if mode == "all":
        rows += [(name + "aug_{}".format(z), "aug") for z in range(2)]
    return rows


def oversample_file(images: torch.Tensor, name: str, patient: int, mode, rng):
    """images [C, 1, H, W, Cc] of one training file -> (rows [M, 1, H, W, Cc], names [M]): each cycle followed by its copies.  The bleed
    fraction of every cycle (label pixels >= 1.05 over H*W) comes back in one read; all copies of the file are one ``dataAug_batch``."""
    Cn, _, H, W, _ = images.shape
    counts = (images[:, 0, :, :, 0] >= 1.05).sum(dim=(1, 2)).tolist() if Cn else []
    src, params, order, names = [], [], [], []
    for h in range(Cn):
        order.append(h)
        names.append(name)
        for row_name, kind in oversample_plan(name, patient, counts[h] / (H * W), mode):
            order.append(Cn + len(src))
            names.append(row_name)
            src.append(h)
            params.append(dict(REDUC_ONLY) if kind == "reduc" else draw_aug(rng))
    if not src:
        return images, names
    copies = dataAug_batch(images[:, 0][torch.as_tensor(src, device=images.device)], params)
    rows = torch.cat([images, copies[:, None]])[torch.as_tensor(order, device=images.device)]
    return rows, names


def _stack(images: List[torch.Tensor], names: List[str], seed: int):
    """Concatenate, shuffle with ``seed`` (sklearn.utils.shuffle's order, :476-479) and bring to the host."""
    perm = permutation(len(names), seed)
    if images:
        data = torch.cat(images)[torch.as_tensor(perm, device=images[0].device)].cpu().numpy()
    else:
        data = np.zeros((0, 1, OUT_H, OUT_W, 12), np.float64)
    paths = np.array(names, dtype=str).reshape(-1, 1)[perm]
    return data, paths


def build_arrays(iteration: int, objective: int, rawDataPath: str, *, seed=None, device="cuda", oversample=None):
    """-> (train [N,1,256,80,12] float64, test [M,1,256,80,12] float64, train_paths [N,1] str, test_paths [M,1] str), the four arrays
    ``output2DImages`` saves.  The final shuffle uses ``seed`` for the training rows and ``seed // 17`` for the test rows (:475-479).
    ``oversample`` "bleed" or "all" appends the copies of ``oversample_plan`` after each TRAINING row (test rows are never copied), their
    draws from ``random.Random(seed)`` in processing order; None keeps the arrays as they are without the block."""
    if oversample not in OVERSAMPLE_MODES:
        raise ValueError(f"oversample must be one of {OVERSAMPLE_MODES}, got {oversample!r}")
    if seed is None:
        seed = np.random.randint(0, int(1e5))
    rng = random.Random(seed)
    tr, te, tr_names, te_names = [], [], [], []
    for name, _, is_test in patient_plan(iteration, rawDataPath):
        folder = os.path.join(rawDataPath, name)
        for file in sorted(os.listdir(folder)):
            if ".mat" not in file:
                continue
            images, pathName = process_file(os.path.join(folder, file), objective, device)
            if is_test or oversample is None:
                (te if is_test else tr).append(images)
                (te_names if is_test else tr_names).extend([pathName] * images.shape[0])
            else:
                rows, row_names = oversample_file(images, pathName, int(name[-3:]), oversample, rng)
                tr.append(rows)
                tr_names.extend(row_names)
    train, train_paths = _stack(tr, tr_names, seed)
    test, test_paths = _stack(te, te_names, seed // 17)
    return train, test, train_paths, test_paths


def output2DImages(iteration, objective, rawDataPath, savePath, *, seed=None, oversample=None):
    """The reference's output2DImages (:249-493): ``savePath/brainMask`` (objective 0) or ``savePath/bleed`` (objective 1) gets
    TrainingData.npy, TestingData.npy, TrainingPaths.npy and TestingPaths.npy.  A folder that already holds files is left as it is.
    ``oversample``: see ``build_arrays``."""
    dataFolder = os.path.join(savePath, "brainMask" if objective == 0 else "bleed")
    if os.path.isdir(dataFolder) and len(os.listdir(dataFolder)) != 0:
        print(str(dataFolder) + " contains data. End of data processing")
        return
    os.makedirs(dataFolder, exist_ok=True)
    train, test, train_paths, test_paths = build_arrays(iteration, objective, rawDataPath, seed=seed, oversample=oversample)
    print("training {}".format(train.shape))
    print("testing {}".format(test.shape))
    print("saved in : {}".format(savePath))
    np.save(os.path.join(dataFolder, "TrainingData.npy"), train)
    np.save(os.path.join(dataFolder, "TestingData.npy"), test)
    np.save(os.path.join(dataFolder, "TrainingPaths.npy"), train_paths)
    np.save(os.path.join(dataFolder, "TestingPaths.npy"), test_paths)


# ---------------------------------------------------------------------------------------------------------- the display axis
def _area_weights(ssize: int, dsize: int, box: bool) -> np.ndarray:
    """[dsize, ssize] float64 matrix of cv2's INTER_AREA weights along one axis (float32 coefficients)."""
    inv = dsize / ssize
    scale = 1.0 / inv
    Wt = np.zeros((dsize, ssize), np.float64)
    for d in range(dsize):
        if box:
            fs1 = d * scale
            fs2 = fs1 + scale
            cell = min(scale, ssize - fs1)
            s2 = min(math.floor(fs2), ssize - 1)
            s1 = min(math.ceil(fs1), s2)
            if s1 - fs1 > 1e-3:
                Wt[d, s1 - 1] += np.float32((s1 - fs1) / cell)
            for s in range(s1, s2):
                Wt[d, s] += np.float32(1.0 / cell)
            if fs2 - s2 > 1e-3:
                Wt[d, s2] += np.float32(min(min(fs2 - s2, 1.0), cell) / cell)
        else:
            s = math.floor(d * scale)
            f = np.float32((d + 1) - (s + 1) * inv)
            f = np.float32(0.0) if f <= 0 else f - np.float32(math.floor(f))
            if s >= ssize - 1:
                Wt[d, ssize - 1] = 1.0
            else:
                Wt[d, s], Wt[d, s + 1] = np.float32(1.0) - f, f
    return Wt


def resize_area(src, dsize_hw=(OUT_H, OUT_W)) -> np.ndarray:
    """cv2.resize(src, (W, H), interpolation=INTER_AREA) of a 2-D array, in float64 (see the module docstring)."""
    src = np.asarray(src, np.float64)
    if src.ndim != 2:
        raise ValueError(f"resize_area takes a 2-D array, got {src.shape}")
    (H, W), (h, w) = src.shape, dsize_hw
    box = H >= h and W >= w
    return _area_weights(H, h, box) @ src @ _area_weights(W, w, box).T


def FetchPolarAxis(datapath, axisPath):
    """:86-100: the file's xAxis and zAxis resized to 256x80 with INTER_AREA, +100 and -4, saved as axis/xAxis.npy and axis/yAxis.npy."""
    from scipy.io import loadmat
    mat = loadmat(datapath)
    xaxis = resize_area(mat["xAxis"]) + 100
    yaxis = resize_area(mat["zAxis"]) - 4
    print("saved axis info in : {}".format(axisPath))
    np.save(os.path.join(axisPath, "xAxis.npy"), xaxis)
    np.save(os.path.join(axisPath, "yAxis.npy"), yaxis)


def main(argv=None):
    """:496-515: both objectives, then the display axis from a file of patient DoD009."""
    ap = argparse.ArgumentParser(description="Raw .mat scans -> the training / test arrays of the brain-mask and bleed models.")
    ap.add_argument("raw", help="folder of patient folders (DoD001, ...) holding .mat files")
    ap.add_argument("save", help="output folder: brainMask/, bleed/ and axis/ are created in it")
    ap.add_argument("--iteration", type=int, default=1, help="patients with index %% 10 == iteration %% 10 form the test set")
    ap.add_argument("--seed", type=int, default=None, help="seed of the final shuffle (default: drawn, as in the reference)")
    ap.add_argument("--oversample", choices=("bleed", "all"), default=None,
                    help="append augmented copies of training rows: of IPH patients and bleed-bearing records, 'all': of every record")
    a = ap.parse_args(argv)
    os.makedirs(a.save, exist_ok=True)
    output2DImages(a.iteration, 0, a.raw, a.save, seed=a.seed, oversample=a.oversample)
    output2DImages(a.iteration, 1, a.raw, a.save, seed=a.seed, oversample=a.oversample)
    axisPath = os.path.join(a.save, "axis")
    if not os.path.isdir(axisPath):
        os.mkdir(axisPath)
        rng = random if a.seed is None else random.Random(a.seed)
        files = sorted(os.listdir(os.path.join(a.raw, "DoD009")))
        FetchPolarAxis(os.path.join(a.raw, "DoD009", rng.choice(files)), axisPath)


if __name__ == "__main__":
    main()
