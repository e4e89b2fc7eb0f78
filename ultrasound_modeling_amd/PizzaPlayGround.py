"""The reference's IPH-only ("pizza") bleed set builder ``PizzaPlayGround.output2DImages`` (PizzaPlayGround.py:38-202): the raw ``.mat``
scans of the intraparenchymal-haemorrhage patients -> ``bleed/`` ``TrainingData.npy`` / ``TestingData.npy`` [N,1,256,80,12] and their
paths, the input of the reference's latest evaluation (``DisplayInference.py`` reads ``pizza_IPH/9/TestingData.npy``).  Channel 0 is the
label, 1-10 the normalised displacement frames of one cardiac cycle, 11 the B-mode image, as in ``DataFilePlayGround``.

Rules, as the reference executes them:
  * patients: every entry of ``rawDataPath``, sorted, shuffled with random_state 20 (:157-159); a patient is processed iff
    ``int(name[-3:])`` is in ``IPH_PATIENTS`` and not in ``BAD_PATIENTS`` (:170; 69 is in both); it is a test patient iff
    index % 10 == iteration % 10, where the index counts every entry, skipped ones included (:138);
  * fields ``bloodMaskThick``, ``brainMask``, ``bModeNorm`` (read first), then ``displacement`` and ``hrTimes``; no ``normalMask``.  An
    empty ``bloodMaskThick`` (``len == 0``) ends the walk of that patient's files (``break``, :68-69);
  * every cycle is one row; the label is ``float32(bloodMaskThick + 1)`` resized in float32 and 0 where the resized brain mask is 0, with
    no blur (:92-97, ``usseg_prep_label_thick`` order 0); the displacement frames are gated like DataFilePlayGround's objective 1;
  * the final shuffle uses ``seed`` for the training rows and ``seed // 17`` for the test rows (:186-190).

The numeric work is DataFilePlayGround's chain on the device (csrc/prep.hip) with ``usseg_prep_label_thick`` in place of the blurred
label: per file one host-to-device copy, then the plane statistics, the label and gate, and the assembly on the current stream.

Deliberate deviations from the reference (besides DataFilePlayGround's: one process, sorted files within a patient, float64 inputs,
``ValueError`` naming a malformed file, a drawn or given ``seed``):
  * the raw and save folders are arguments (the reference's ``__main__`` names an undefined ``rawDataPath`` and an undefined ``FetchAxis``;
    the port calls ``FetchPolarAxis``), and the ``bleed/`` folder is created if it is missing;
  * ``main`` takes ``--seed`` for the final shuffle and the random axis file.
"""
from __future__ import annotations

import argparse
import os
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .DataFilePlayGround import OUT_H, OUT_W, PATIENT_SEED, FetchPolarAxis, _check, _gather, _require, _stack, _upload, permutation

IPH_PATIENTS = (8, 9, 10, 12, 22, 47, 53, 62, 66, 67, 69, 74, 75, 78, 85, 89, 93, 101, 105, 107, 110, 112, 113, 120, 121, 126, 129, 130,
                133)                                                                              # :47-48
BAD_PATIENTS = (27, 28, 35, 36, 38, 49, 69, 90)                                                   # :50
READ_FIRST = ("bloodMaskThick", "brainMask", "bModeNorm")                                         # :64-66, before the empty test


def empty_mask(m) -> bool:
    """The reference's ``len(bloodMask) == 0`` on ``np.array(list(mat['bloodMaskThick']))``: no rows."""
    m = np.asarray(m)
    return m.ndim > 0 and m.shape[0] == 0


def patient_plan(iteration: int, rawDataPath: str) -> List[Tuple[str, int, bool]]:
    """The patients ``output2DImages`` processes, in its order: (folder name, index in the shuffled list, goes to the test set)."""
    names = np.sort(os.listdir(rawDataPath))
    names = names[permutation(len(names), PATIENT_SEED)]
    plan = []
    for index, name in enumerate(names):
        num = int(name[-3:])
        if num in BAD_PATIENTS or num not in IPH_PATIENTS:
            continue
        plan.append((str(name), index, index % 10 == iteration % 10))
    return plan


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


def process_file(path: str, device="cuda") -> Optional[Tuple[torch.Tensor, str]]:
    """One ``.mat`` file -> (images, name): images a device float64 [C,1,256,80,12], one per cardiac cycle (:59-145); name = the file
    name's first 17 characters (:62).  None when the file's bloodMaskThick is empty: the caller ends the patient's walk there.
    Enqueued on the current stream."""
    loaded = _load(path)
    if loaded is None:
        return None
    frames, bmode, brain, blood = loaded
    name = os.path.basename(path)[0:17]
    device = torch.device(device)
    if frames.shape[0] == 0:
        return torch.empty((0, 1, OUT_H, OUT_W, 12), dtype=torch.float64, device=device), name
    frames_d, bmode_d, brain_d, blood_d = _upload([frames, bmode, brain, blood], device)    # the one host-to-device copy
    stats = ops.prep_cycle_stats(frames_d)
    label, gate = ops.prep_label_thick(brain_d, blood_d, 0)
    return ops.prep_assemble(frames_d, stats, bmode_d, label, gate, 1), name


def build_arrays(iteration: int, rawDataPath: str, *, seed=None, device="cuda"):
    """-> (train [N,1,256,80,12] float64, test [M,1,256,80,12] float64, train_paths [N,1] str, test_paths [M,1] str), the four arrays
    ``output2DImages`` saves.  The final shuffle uses ``seed`` for the training rows and ``seed // 17`` for the test rows."""
    if seed is None:
        seed = np.random.randint(0, int(1e5))
    tr, te, tr_names, te_names = [], [], [], []
    for name, _, is_test in patient_plan(iteration, rawDataPath):
        folder = os.path.join(rawDataPath, name)
        for file in sorted(os.listdir(folder)):
            if ".mat" not in file:
                continue
            res = process_file(os.path.join(folder, file), device)
            if res is None:
                break                                                  # an empty bloodMaskThick ends the patient (:68-69)
            images, pathName = res
            (te if is_test else tr).append(images)
            (te_names if is_test else tr_names).extend([pathName] * images.shape[0])
    train, train_paths = _stack(tr, tr_names, seed)
    test, test_paths = _stack(te, te_names, seed // 17)
    return train, test, train_paths, test_paths


def output2DImages(iteration, rawDataPath, savePath, *, seed=None):
    """The reference's output2DImages (:38-202): ``savePath/bleed`` gets TrainingData.npy, TestingData.npy, TrainingPaths.npy and
    TestingPaths.npy (overwritten if present, as the reference does)."""
    dataFolder = os.path.join(savePath, "bleed")
    os.makedirs(dataFolder, exist_ok=True)
    train, test, train_paths, test_paths = build_arrays(iteration, rawDataPath, seed=seed)
    print("training {}".format(train.shape))
    print("testing {}".format(test.shape))
    print("saved in : {}".format(savePath))
    np.save(os.path.join(dataFolder, "TrainingData.npy"), train)
    np.save(os.path.join(dataFolder, "TestingData.npy"), test)
    np.save(os.path.join(dataFolder, "TrainingPaths.npy"), train_paths)
    np.save(os.path.join(dataFolder, "TestingPaths.npy"), test_paths)


def fetch_random_axis(rawDataPath, savePath, seed=None):
    """The reference's ``__main__`` tail (:208-219): unless ``savePath/axis`` exists, the display axis of a random file of a random
    patient (``random.choice`` over the sorted listings; ``seed`` makes the choice reproducible)."""
    axisPath = os.path.join(savePath, "axis")
    if os.path.isdir(axisPath):
        return
    os.mkdir(axisPath)
    rng = random if seed is None else random.Random(seed)
    patient = rng.choice(sorted(os.listdir(rawDataPath)))
    file = rng.choice(sorted(os.listdir(os.path.join(rawDataPath, patient))))
    FetchPolarAxis(os.path.join(rawDataPath, patient, file), axisPath)


def main(argv=None):
    """:205-219: the pizza bleed set, then the display axis."""
    ap = argparse.ArgumentParser(description="Raw .mat scans of the IPH patients -> the bleed/ training and test arrays (the pizza set).")
    ap.add_argument("raw", help="folder of patient folders (DoD008, ...) holding .mat files")
    ap.add_argument("save", help="output folder, e.g. PROCESSED/pizza_IPH/9: bleed/ and axis/ are created in it")
    ap.add_argument("--iteration", type=int, default=1, help="patients with index %% 10 == iteration %% 10 form the test set")
    ap.add_argument("--seed", type=int, default=None, help="seed of the final shuffle and the axis file (default: drawn, as in the reference)")
    a = ap.parse_args(argv)
    os.makedirs(a.save, exist_ok=True)
    output2DImages(a.iteration, a.raw, a.save, seed=a.seed)
    fetch_random_axis(a.raw, a.save, a.seed)


if __name__ == "__main__":
    main()
