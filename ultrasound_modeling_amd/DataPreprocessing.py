"""The authors' rewritten dataset builder ``DataPreprocessing.py`` (:82-234): a folder of patients' raw ``.mat`` scans -> ``brain/``
(objective 0) and ``bleed/`` (objective 1) ``TrainingData.npy`` / ``TestingData.npy`` [N,1,256,80,12] and their paths.  Channel 0 is the
label, 1-10 the normalised displacement frames of one cardiac cycle, 11 the B-mode image, as in ``DataFilePlayGround``.

Rules, as the reference executes them:
  * every patient folder is used; there is no bad-patient or IPH filter;
  * fields ``normalMask`` (read, unused), ``bloodMaskThick``, ``brainMask``, ``bModeNorm`` (read first), then ``displacement`` and
    ``hrTimes``.  An empty ``bloodMaskThick`` (``len == 0``) ends the walk of that patient's files (``break``, :126-127);
  * objective 0: label 1 where the resized brain mask is non-zero, else 0, and no gate on the frames (:141-142); objective 1: the resized
    ``bloodMaskThick`` (fp64) + 1, as float32, 0 where the resized brain mask is 0 (:144-146, ``usseg_prep_label_thick`` order 1), and
    the frames gated (:160-163);
  * **only the last cycle of each file is kept**: ``data.append`` sits after the cycle loop (:168-169), so the sample it appends is the
    one the last iteration built, with the path ``file[0:17] + "_cycle" + str(C-1)``.  Only that cycle's frames and B-mode slice go to the
    device; every cycle's window is still checked, as the reference slices them all (:57-59);
  * the split is ``train_test_split(data, names, test_size=0.5, random_state=42)`` over the patients (the axis the reference's stacking
    gives): ``RandomState(42).permutation(P)``, the first ``ceil(P/2)`` patients are the test side, the rest the training side, each in
    that order.  It raises sklearn's error when the training side would be empty (P < 2).

The numeric work is DataFilePlayGround's chain on the device (csrc/prep.hip): per file one host-to-device copy, then the plane statistics,
the label and gate (``usseg_prep_label`` objective 0 or ``usseg_prep_label_thick`` order 1) and the assembly on the current stream.

Deliberate deviations from the reference (besides DataFilePlayGround's: float64 inputs, ``ValueError`` naming a malformed file):
  * patients and their files are processed in sorted order, not ``os.listdir`` order;
  * the output is float64 [N,1,256,80,12] with paths [N,1]; each side holds its patients' rows in order.  The reference stacks a ragged
    per-patient list, which NumPy refuses unless every patient has the same file count, and then yields [P,F,256,80,12], a layout no reader
    here accepts;
  * a file with no cycle contributes no row (the reference re-appends the previous file's sample or raises ``NameError``);
  * the raw and save folders are arguments, the output folders' parents are created, and ``main`` takes ``--seed`` for the random axis
    file.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .DataFilePlayGround import OUT_H, OUT_W, FetchPolarAxis, _check, _gather, _require, _upload
from .PizzaPlayGround import empty_mask, fetch_random_axis

FetchAxis = FetchPolarAxis                                                       # :23-37, the same function
READ_FIRST = ("normalMask", "bloodMaskThick", "brainMask", "bModeNorm")          # :121-124, before the empty test


def _load(path: str):
    """Read and check one file; -> None for an empty bloodMaskThick, else host float64 (frames [C,10,H0,W0], bmode [C,Hq,Wq,F], brain,
    blood)."""
    from scipy.io import loadmat
    mat = loadmat(path)
    _require(path, mat, READ_FIRST)
    if empty_mask(mat["bloodMaskThick"]):
        return None
    _require(path, mat, ("displacement", "hrTimes"))
    disp, hr, bmode, (brain, blood) = _check(path, mat, ("brainMask", "bloodMaskThick"))
    return _gather(path, disp, hr, bmode) + (brain, blood)


def process_file(path: str, objective: int, device="cuda") -> Optional[Tuple[torch.Tensor, Optional[str]]]:
    """One ``.mat`` file -> (images, name): images a device float64 [1,1,256,80,12], the file's last cardiac cycle (:129-169), and
    name = ``file[0:17] + "_cycle" + str(C-1)``; a file with no cycle gives [0,1,256,80,12] and None.  None when the file's
    bloodMaskThick is empty: the caller ends the patient's walk there.  Enqueued on the current stream."""
    if objective not in (0, 1):
        raise ValueError(f"objective must be 0 (brain mask) or 1 (bleed), got {objective}")
    loaded = _load(path)
    if loaded is None:
        return None
    frames, bmode, brain, blood = loaded
    device = torch.device(device)
    C = frames.shape[0]
    if C == 0:
        return torch.empty((0, 1, OUT_H, OUT_W, 12), dtype=torch.float64, device=device), None
    name = os.path.basename(path)[0:17] + "_cycle" + str(C - 1)
    parts = [np.ascontiguousarray(frames[C - 1:]), np.ascontiguousarray(bmode[C - 1:]), brain] + ([blood] if objective == 1 else [])
    views = _upload(parts, device)                                                     # the one host-to-device copy
    frames_d, bmode_d, brain_d = views[:3]
    stats = ops.prep_cycle_stats(frames_d)
    if objective == 0:
        label, gate = ops.prep_label(brain_d, 0)
    else:
        label, gate = ops.prep_label_thick(brain_d, views[3], 1)
    return ops.prep_assemble(frames_d, stats, bmode_d, label, gate, objective), name


def process_data(path: str, objective: int, device="cuda") -> Tuple[torch.Tensor, List[str]]:
    """One patient folder (:105-171) -> (device float64 [n,1,256,80,12], the n row names), its files in sorted order."""
    data, fileNames = [], []
    for file in sorted(os.listdir(path)):
        if ".mat" not in file:
            continue
        res = process_file(os.path.join(path, file), objective, device)
        if res is None:
            break                                                      # an empty bloodMaskThick ends the patient (:126-127)
        images, name = res
        if images.shape[0]:
            data.append(images)
            fileNames.append(name)
    if not data:
        return torch.empty((0, 1, OUT_H, OUT_W, 12), dtype=torch.float64, device=torch.device(device)), fileNames
    return torch.cat(data), fileNames


def process_patients(path: str, objective: int, device="cuda"):
    """Every patient folder of ``path`` in sorted order (:82-102) -> (per-patient data list, per-patient name lists)."""
    patients_data, file_list = [], []
    for patient in sorted(os.listdir(path)):
        data, fileNames = process_data(os.path.join(path, patient), objective, device)
        patients_data.append(data)
        file_list.append(fileNames)
    return patients_data, file_list


def split_patients(P: int, test_size: float = 0.2, random_state: int = 42) -> Tuple[np.ndarray, np.ndarray]:
    """-> (train, test) patient indices of ``sklearn.model_selection.train_test_split`` over P items with a float ``test_size``:
    ``RandomState(random_state).permutation(P)``, the first ``ceil(test_size*P)`` the test side, the rest the training side."""
    n_test = math.ceil(test_size * P)
    n_train = P - n_test
    if n_train <= 0:
        raise ValueError("With n_samples={}, test_size={} and train_size={}, the resulting train set will be empty. Adjust any of the "
                         "aforementioned parameters.".format(P, test_size, None))
    perm = np.random.RandomState(random_state).permutation(P)
    return perm[n_test:], perm[:n_test]


def _rows(data, nameList, idx):
    parts = [data[i] for i in idx if data[i].shape[0]]
    rows = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 1, OUT_H, OUT_W, 12), np.float64)
    names = [n for i in idx for n in nameList[i]]
    return rows, np.array(names, dtype=str).reshape(-1, 1)


def split_rows(data, nameList, test_size=0.2, random_state=42):
    """Per-patient data and names -> (train, test, train_paths, test_paths) host arrays, split by patient as ``split_patients``."""
    train_idx, test_idx = split_patients(len(data), test_size, random_state)
    train, train_paths = _rows(data, nameList, train_idx)
    test, test_paths = _rows(data, nameList, test_idx)
    return train, test, train_paths, test_paths


def split_data(data, nameList, savePath, test_size=0.2, random_state=42):
    """:174-195: split by patient and save TrainingData.npy, TestingData.npy, TrainingPaths.npy and TestingPaths.npy in savePath."""
    train, test, train_paths, test_paths = split_rows(data, nameList, test_size, random_state)
    np.save(os.path.join(savePath, "TrainingData.npy"), train)
    np.save(os.path.join(savePath, "TestingData.npy"), test)
    np.save(os.path.join(savePath, "TrainingPaths.npy"), train_paths)
    np.save(os.path.join(savePath, "TestingPaths.npy"), test_paths)


def build_arrays(objective: int, rawDataPath: str, *, device="cuda"):
    """-> (train, test, train_paths, test_paths) as ``main`` saves them for ``objective`` (test_size 0.5, random_state 42)."""
    return split_rows(*process_patients(rawDataPath, objective, device), test_size=0.5)


def main(argv=None):
    """:198-234: objective 0 into brain/, objective 1 into bleed/, then the display axis."""
    ap = argparse.ArgumentParser(description="Raw .mat scans -> the brain/ and bleed/ training and test arrays (last cycle of each file).")
    ap.add_argument("raw", help="folder of patient folders holding .mat files")
    ap.add_argument("save", help="output folder: brain/, bleed/ and axis/ are created in it")
    ap.add_argument("--seed", type=int, default=None, help="seed of the random axis file (default: drawn, as in the reference)")
    a = ap.parse_args(argv)
    for objective, folder in ((0, "brain"), (1, "bleed")):
        out = os.path.join(a.save, folder)
        os.makedirs(out, exist_ok=True)
        data, fileList = process_patients(a.raw, objective)
        print("patients {}, rows {}".format(len(data), sum(int(d.shape[0]) for d in data)))
        split_data(data, fileList, out, test_size=0.5)
    fetch_random_axis(a.raw, a.save, a.seed)


if __name__ == "__main__":
    main()
