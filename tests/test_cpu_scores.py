"""Per-image and per-patient scores with bleed areas in physical units, without a GPU: ``metrics.ScanGeometry``'s areas against the analytic
area of a sector scan and its fixed-point tables against their documented bounds; ``patient_of`` / ``grouped`` / ``summarize`` on hand tables;
the restatement's bootstrap draws against hand-computed indices; the second header (include/usseg_scores.h), the symbols it declares and
every argument check of csrc/scores.hip before any launch; and the evaluator's CSV writers and ``main`` flags on a small synthetic run with the
GPU wrappers replaced by the restatement (tests/scores_restatement.py)."""
import csv
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import components_restatement as CR
import scores_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the geometry
@pytest.mark.parametrize("H,W,r0,dr,t0,dt", [(256, 80, 20.0, 0.25, -0.5, 0.0125), (7, 5, 3.0, 1.5, 0.2, 0.11), (2, 2, 1.0, 0.5, -0.1, 0.2)])
def test_areas_of_a_sector_scan_equal_r_dr_sin_dtheta(H, W, r0, dr, t0, dt):
    """x = r sin(theta), y = r cos(theta): the central differences give dXi = dr sin(theta), dYi = dr cos(theta), dXj = r cos(theta) sin(dt),
    dYj = -r sin(theta) sin(dt), so |dXi dYj - dXj dYi| = r dr sin(dt).  The one-sided rows give the same dXi, dYi (x and y are linear in r);
    the one-sided columns give dXj = 2 r cos(theta + dt/2) sin(dt/2), dYj = -2 r sin(theta + dt/2) sin(dt/2), and the product again
    2 r dr sin(dt/2) cos(dt/2) = r dr sin(dt).  So the formula holds at EVERY sample.  Bound: a difference of two coordinates of magnitude
    <= m = max(|X|, |Y|) carries an absolute error of a few 2^-53 m against a true size of at least min(dr, r0 sin(dt)) - the smaller of the
    two cell edges - so each factor is off by that ratio relatively; 64 covers the inputs' own roundings, the four differences, the two
    products and their subtraction."""
    from ultrasound_modeling_amd.metrics import ScanGeometry
    X, Y = SR.polar_axes(H, W, r0, dr, t0, dt)
    g = ScanGeometry(X, Y)
    r = r0 + dr * np.arange(H, dtype=np.float64)[:, None]
    want = np.broadcast_to(r * dr * math.sin(dt), (H, W))
    bound = 64 * 2.0 ** -53 * max(np.abs(X).max(), np.abs(Y).max()) / min(dr, r0 * math.sin(dt))
    rel = np.abs(g.area - want) / want
    print(f"{H}x{W}: largest relative error {rel.max():.3e}, bound {bound:.3e}")
    assert g.area.dtype == np.float64 and g.area.shape == (H, W) and rel.max() <= bound
    assert g.area[-1, 0] > 1.5 * g.area[0, 0] or H < 7                 # a deep pixel covers more than a shallow one


def test_areas_known_answers_and_refusals():
    from ultrasound_modeling_amd.metrics import ScanGeometry
    X, Y = np.meshgrid(np.arange(9.0), np.arange(6.0))
    g = ScanGeometry(X, Y)
    assert np.array_equal(g.area, np.ones((6, 9))) and g.quantum == 1.0 / (2 ** 20 - 1) and (g.wq == 2 ** 20 - 1).all()
    assert np.array_equal(ScanGeometry(Y, X).area, np.ones((6, 9)))   # the mirrored orientation: the absolute value
    g2 = ScanGeometry([[0.0, 0.0], [3.0, 3.0]], [[0.0, 2.0], [0.0, 2.0]])
    assert np.array_equal(g2.area, np.full((2, 2), 6.0)) and g2.xq.tolist() == [[0, 0], [65535, 65535]] and g2.yq.tolist() == [[0, 65535], [0, 65535]]
    # the axes are NOT cast: a grid that astype(int) would collapse keeps its area
    gf = ScanGeometry(X * 0.25, Y * 0.25)
    assert np.allclose(gf.area, 0.0625, rtol=1e-15) and (X * 0.25).astype(int)[:, :4].max() == 0
    assert "astype(int)" in ScanGeometry.__doc__ and "display quirk" in ScanGeometry.__doc__
    for bad in ((np.zeros((3, 3)), np.zeros((3, 3))),                  # collapsed to a point
                (X, X),                                                # collapsed to a line
                (X[:1], Y[:1]), (X[:, :1], Y[:, :1]), (X, Y[:5]), (X.ravel(), Y.ravel()),
                (np.where(X == 2, np.nan, X), Y), (np.where(X == 2, np.inf, X), Y),
                (X * 1e200, Y * 1e200)):                               # the area overflows
        with pytest.raises(ValueError):
            ScanGeometry(*bad)
    # a zero span along one axis cannot have area, but the quantiser itself maps it to step 1, q 0
    assert ScanGeometry._quantise(np.full((2, 3), 7.5)) [1] == 1.0 and not ScanGeometry._quantise(np.full((2, 3), 7.5))[2].any()


def test_fixed_point_tables_and_round_trips():
    from ultrasound_modeling_amd.metrics import ScanGeometry
    X, Y = SR.polar_axes(67, 29)
    g = ScanGeometry(X, Y)
    assert g.wq.dtype == np.uint32 and g.wq.max() == 2 ** 20 - 1 and g.wq.min() >= 1
    assert g.quantum == g.area.max() / (2 ** 20 - 1) and np.array_equal(g.wq, np.rint(g.area / g.quantum).astype(np.uint32))
    for q, V, lo, step in ((g.xq, X, g.x_min, g.xstep), (g.yq, Y, g.y_min, g.ystep)):
        assert q.dtype == np.int32 and q.min() == 0 and q.max() == 65535
        assert step == (V.max() - V.min()) / 65535 and lo == V.min()
        assert np.abs(lo + step * q - V).max() <= step / 2 * (1 + 1e-9)
    assert np.abs(g.wq * g.quantum - g.area).max() <= g.quantum / 2 * (1 + 1e-9)
    rng = np.random.default_rng(5)
    for density in (0.02, 0.5, 1.0):
        sel = rng.random(X.shape) < density
        sel[3, 4] = True
        n = int(sel.sum())
        w = g.wq[sel].astype(np.int64)
        sw, swx, swy = int(w.sum()), int((w * g.xq[sel]).sum()), int((w * g.yq[sel]).sum())
        assert abs(float(g.area_of(sw)) - g.area[sel].sum()) <= n * g.quantum / 2 * (1 + 1e-9)
        assert abs(float(g.x_of(swx, sw)) - float((w * X[sel]).sum() / sw)) <= g.xstep / 2 * (1 + 1e-9)
        assert abs(float(g.y_of(swy, sw)) - float((w * Y[sel]).sum() / sw)) <= g.ystep / 2 * (1 + 1e-9)
    assert np.isnan(g.x_of(0, 0)) and np.isnan(g.y_of(0, 0)) and float(g.area_of(0)) == 0.0
    assert float(g.x_at(0)) == g.x_min and abs(float(g.y_at(65535)) - Y.max()) <= 1e-12 * abs(Y.max())
    wq, xq, yq = g.tables("cpu")
    assert all(t.dtype == torch.int32 and t.shape == (67, 29) for t in (wq, xq, yq)) and g.tables("cpu")[0] is wq
    assert np.array_equal(wq.numpy(), g.wq.astype(np.int32)) and np.array_equal(xq.numpy(), g.xq)
    # the overflow budget of the header: the largest sum one image can form fits int64
    assert (2 ** 20 - 1) * 65535 * ScanGeometry.MAX_DIM ** 2 < 2 ** 62
    with pytest.raises(ValueError):
        ScanGeometry(np.zeros((2, 8193)), np.zeros((2, 8193)))


# ------------------------------------------------------------------------------------------------ tables by hand
HAND = dict(tp=[3, 0, 0, 5], fp=[1, 0, 0, 5], fn=[2, 0, 4, 0], tn=[10, 16, 12, 6])
HAND_W = dict(w_true=[10, 0, 8, 10], w_pred=[8, 0, 0, 20], w_tp=[6, 0, 0, 10], quantum=0.5)


def test_patient_of():
    from ultrasound_modeling_amd.metrics import patient_of
    assert patient_of("DoD012_frame3") == "012" and patient_of("/data/DoD7/x/DoD9.npy") == "7" and patient_of(np.str_("aDoD33b")) == "33"
    assert patient_of(b"DoD5_f") == "5"
    assert patient_of("frame3") == "frame3" and patient_of("DoDx") == "DoDx"          # no match: its own group
    assert patient_of("P12_f3", pattern=r"P\d+") == "P12" and patient_of("P12_f3", pattern=r"P(\d+)_f(\d+)") == "12"


def test_scores_grouped_and_summarize_by_hand():
    from ultrasound_modeling_amd import metrics as M
    t = M.scores_from_counts(**HAND)
    nan = float("nan")
    assert np.array_equal(t["dice"], [6 / 9, nan, 0.0, 10 / 15], equal_nan=True)
    assert np.array_equal(t["iou"], [3 / 6, nan, 0.0, 5 / 10], equal_nan=True)
    assert np.array_equal(t["sensitivity"], [3 / 5, nan, 0.0, 1.0], equal_nan=True)
    assert np.array_equal(t["precision"], [3 / 4, nan, nan, 0.5], equal_nan=True)      # image 2 predicts nothing: no precision
    assert all(t[c].dtype == np.int64 for c in M.SCORE_COUNTS) and "area_true" not in t
    g = M.grouped(t, ["A", "A", "B", "B"])
    assert g["groups"] == ["A", "B"] and g["n_images"].tolist() == [2, 2]
    assert (g["tp"].tolist(), g["fp"].tolist(), g["fn"].tolist(), g["tn"].tolist()) == ([3, 5], [1, 5], [2, 4], [26, 18])
    assert g["dice"].tolist() == [6 / 9, 10 / 19] and g["precision"].tolist() == [3 / 4, 5 / 10]
    g1 = M.grouped(t, ["B", "x", "A", "B"])                                            # first appearance orders the rows
    assert g1["groups"] == ["B", "x", "A"] and g1["tp"].tolist() == [8, 0, 0] and np.isnan(g1["dice"][1]) and g1["dice"][2] == 0.0
    with pytest.raises(ValueError):
        M.grouped(t, ["A", "B"])
    s = M.summarize(t)
    assert s["n_images"] == 4 and "bootstrap" not in s and "bland_altman" not in s
    assert (s["pooled"]["tp"], s["pooled"]["fp"], s["pooled"]["fn"], s["pooled"]["tn"]) == (8, 6, 6, 44)
    assert s["pooled"]["dice"] == 16 / 28 and s["pooled"]["iou"] == 8 / 20 and s["pooled"]["sensitivity"] == 8 / 14 and s["pooled"]["precision"] == 8 / 14
    assert s["defined"] == {"dice": 3, "iou": 3, "sensitivity": 3, "precision": 2}
    assert s["mean"]["dice"] == np.mean([6 / 9, 0.0, 10 / 15]) and s["median"]["dice"] == np.median([6 / 9, 0.0, 10 / 15])
    assert s["mean"]["precision"] == (0.75 + 0.5) / 2 and s["median"]["sensitivity"] == 3 / 5
    # with areas: quantum 0.5
    ta = M.scores_from_counts(**HAND, **HAND_W)
    assert ta["area_true"].tolist() == [5.0, 0.0, 4.0, 5.0] and ta["area_pred"].tolist() == [4.0, 0.0, 0.0, 10.0] and ta["area_tp"].tolist() == [3.0, 0.0, 0.0, 5.0]
    assert np.array_equal(ta["area_dice"], [12 / 18, nan, 0.0, 20 / 30], equal_nan=True) and ta["area_error"].tolist() == [-1.0, 0.0, -4.0, 5.0]
    sa = M.summarize(ta, groups=["A", "A", "B", "B"])
    ba = sa["bland_altman"]
    sd = math.sqrt((1 + 0 + 16 + 25) / 3)
    assert ba["bias"] == 0.0 and ba["n"] == 4 and abs(ba["sd"] - sd) < 1e-15 and ba["lower"] == -1.96 * ba["sd"] and ba["upper"] == 1.96 * ba["sd"]
    assert sa["n_groups"] == 2 and sa["pooled"]["area_dice"] == 32 / 56 and sa["pooled"]["area_error"] == 0.0 and sa["defined"]["area_dice"] == 3
    ga = M.grouped(ta, ["A", "A", "B", "B"])
    assert ga["w_true"].tolist() == [10, 18] and ga["area_error"].tolist() == [-1.0, 1.0] and ga["area_dice"].tolist() == [12 / 18, 20 / 38]
    # an empty run and a run in which nothing is defined
    e = M.summarize(M.scores_from_counts([], [], [], []))
    assert e["n_images"] == 0 and np.isnan(e["pooled"]["dice"]) and np.isnan(e["mean"]["dice"]) and e["defined"]["dice"] == 0
    z = M.summarize(M.scores_from_counts([0, 0], [0, 0], [0, 0], [9, 9]))
    assert np.isnan(z["mean"]["dice"]) and np.isnan(z["median"]["iou"]) and z["defined"] == {"dice": 0, "iou": 0, "sensitivity": 0, "precision": 0}


def test_the_bootstrap_restatement_draws_the_hand_computed_indices():
    """U = 3, seed = 1: the six z values were computed with NumPy uint64 arithmetic, step by step after the header; their high words times 3,
    shifted down by 32, give the indices."""
    z = [[0x910a2dec89025cc1, 0xbeeb8da1658eec67, 0xf893a2eefb32555e], [0x71c18690ee42c90b, 0x71bb54d8d101b5b9, 0xc34d0bff90150280]]
    hand = [[((v >> 32) * 3) >> 32 for v in row] for row in z]
    assert hand == [[1, 2, 2], [1, 1, 2]]
    assert [[SR.draw_index(1, r, 3, d) for d in range(3)] for r in range(2)] == hand
    rows = np.array([[1, 10], [2, 20], [4, 40]], np.int64)
    assert SR.bootstrap(rows, 2, 1).tolist() == [[2 + 4 + 4, 20 + 40 + 40], [2 + 2 + 4, 20 + 20 + 40]]
    # the first step by hand: z0 = seed + golden * (1 + r*U + d) modulo 2^64
    assert (1 + 0x9E3779B97F4A7C15 * 4) % 2 ** 64 == 0x78DDE6E5FD29F055
    assert SR.bootstrap(rows, 0, 1).shape == (0, 2)
    assert all(0 <= SR.draw_index(s, r, 7, d) < 7 for s in (0, 2 ** 64 - 1) for r in (0, 2 ** 20 - 1) for d in range(7))


def test_bootstrap_intervals_with_the_stand_in(monkeypatch):
    from ultrasound_modeling_amd import metrics as M
    from ultrasound_modeling_amd import ops
    monkeypatch.setattr(ops, "bootstrap_sums", SR.ops_bootstrap_sums)
    # a constant table: every replicate is the same sum, so every interval has zero width at the pooled value
    t = M.scores_from_counts([3] * 5, [1] * 5, [2] * 5, [10] * 5, [10] * 5, [8] * 5, [6] * 5, 0.5)
    s = M.summarize(t, bootstrap=40, seed=9, device="cpu")
    b = s["bootstrap"]
    assert (b["replicates"], b["seed"], b["alpha"], b["unit"], b["units"]) == (40, 9, 0.05, "image", 5)
    assert b["intervals"]["pooled_dice"] == (6 / 9, 6 / 9) and b["intervals"]["area_dice"] == (12 / 18, 12 / 18)
    assert b["intervals"]["area_error_total"] == (-5.0, -5.0) and b["dropped"] == {k: 0 for k in b["intervals"]}
    lo, hi = b["intervals"]["mean_dice"]
    assert lo == hi and abs(lo - 6 / 9) <= 2.0 ** -31                  # rint(dice * 2^30) / 2^30
    # groups: the resampling unit is the patient; the rows are the patients' sums and the per-image Dice rides in two integer columns
    th = M.scores_from_counts(**HAND, **HAND_W)
    names, rows = M.bootstrap_rows(th, ["A", "A", "B", "B"])
    assert names == ("tp", "fp", "fn", "dice_q", "dice_n", "w_tp", "w_true", "w_pred")
    q = lambda v: int(np.rint(v * 2 ** 30))
    assert rows.tolist() == [[3, 1, 2, q(6 / 9), 1, 6, 10, 8], [5, 5, 4, q(0.0) + q(10 / 15), 2, 10, 18, 20]]
    assert M.bootstrap_rows(th)[1][:, 3:5].tolist() == [[q(6 / 9), 1], [0, 0], [0, 1], [q(10 / 15), 1]]
    sg = M.summarize(th, groups=["A", "A", "B", "B"], bootstrap=200, seed=4, alpha=0.1, device="cpu")
    bg = sg["bootstrap"]
    assert bg["unit"] == "group" and bg["units"] == 2
    sums = SR.bootstrap(rows, 200, 4)
    st = M.bootstrap_statistics(names, sums, 0.5)
    for k, (lo, hi) in bg["intervals"].items():
        assert (lo, hi) == tuple(np.quantile(st[k], [0.05, 0.95])), k
    assert set(np.unique(st["pooled_dice"])) == {6 / 9, 16 / 28, 10 / 19}          # AA, AB / BA, BB
    assert bg["intervals"]["pooled_dice"][0] <= sg["pooled"]["dice"] <= bg["intervals"]["pooled_dice"][1]
    # replicates without a defined statistic are dropped and counted: units 1 and 2 alone have no Dice (0 / 0)
    tn = M.scores_from_counts([3, 0, 0], [1, 0, 0], [2, 0, 0], [4, 9, 9])
    sn = M.summarize(tn, bootstrap=300, seed=1, device="cpu")
    sums = SR.bootstrap(M.bootstrap_rows(tn)[1], 300, 1)
    empty = int((sums[:, 0] + sums[:, 1] + sums[:, 2] == 0).sum())
    assert empty > 0 and sn["bootstrap"]["dropped"]["pooled_dice"] == empty == sn["bootstrap"]["dropped"]["mean_dice"]
    assert sn["bootstrap"]["intervals"]["pooled_dice"] == (6 / 9, 6 / 9)
    with pytest.raises(ValueError):
        M.summarize(tn, bootstrap=-1)
    with pytest.raises(ValueError):
        M.summarize(tn, bootstrap=5, alpha=1.5, device="cpu")
    with pytest.raises(ValueError, match="overflow"):
        ops.bootstrap_check_rows(2 ** 61, 3)
    ops.bootstrap_check_rows(2 ** 62 // 3, 3)


# ------------------------------------------------------------------------------------------------ the second header and the C ABI
NEW_SYMBOLS = ("usseg_image_confusion", "usseg_component_measure", "usseg_bootstrap_sums")


def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def test_the_second_header_parses_and_the_first_is_untouched():
    from ultrasound_modeling_amd import _abi
    L, lib = _lib()
    path = os.path.join(ROOT, "include", "usseg_scores.h")
    assert L.SCORES_HEADER_PATH == path
    abi = _abi.parse(open(path).read(), path)
    assert tuple(abi.protos) == NEW_SYMBOLS == L.SCORES_SYMBOLS == tuple(L.SCORES_ABI.protos) and not abi.structs
    assert list(abi.consts.items()) == [("USSEG_SCORES_MEASURE_FIELDS", 8), ("USSEG_SCORES_EMPTY_MIN", 65536), ("USSEG_SCORES_BOOT_MAX_K", 16),
                                        ("USSEG_SCORES_BOOT_MAX", 1 << 20)]
    import ctypes as C
    i32, vp = C.c_int32, C.c_void_p
    assert abi.protos["usseg_image_confusion"] == (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp])
    assert abi.protos["usseg_component_measure"] == (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp])
    assert abi.protos["usseg_bootstrap_sums"] == (C.c_int, [vp, i32, i32, C.c_uint64, i32, vp, vp])
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name not in hdr and name not in L.EXPORTED_SYMBOLS and name not in L._PROTOS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == L.SCORES_ABI.protos[name]             # load() bound the second header's prototypes
    assert (len(L.ABI.protos), len(L.ABI.structs)) == (167, 34) and "usseg_scores" not in hdr
    text = open(path).read()
    for phrase in ("2^20 * 2^16 * 2^26 = 2^62", "U / 2^32", "n * quantum / 2", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                   "index = ((z >> 32) * U) >> 32", "The caller zeroes nothing", "rows = truth, columns =\n *                             prediction",
                   "xq_min = yq_min = 65536", "Ids above cap are skipped"):
        assert phrase in text, phrase
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    assert sum("scores.hip" in line.split() for line in mk.splitlines() if line.startswith(("SRCS", "NOPK_SRCS"))) == 2
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "SCORES_SYMBOLS" in entry                                                    # build() looks for the second header's symbols too
    with pytest.raises(L.UssegError, match="nowhere/usseg_scores.h"):
        L.read_header(os.path.join(ROOT, "nowhere", "usseg_scores.h"))


def _shape_checks(call, err, what):
    for kw in (dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(H=-3)):
        assert call(**kw) == -1 and f"{what}: H and W must lie in [1, 8192]" in err(), kw
    for n in (-1, 65536):
        assert call(N=n) == -1 and f"{what}: 0 <= N <= 65535" in err()
    assert call(N=9, H=8192, W=8192) == -1 and f"{what}: more than 2^29 pixels" in err()


def test_image_confusion_refuses_bad_arguments_before_any_launch():
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(pred=16, truth=16, weight=16, N=1, H=8, W=8, C=2, cm=16, wcm=16, invalid=16):
        return lib.usseg_image_confusion(pred, truth, weight, N, H, W, C, cm, wcm, invalid, None)

    _shape_checks(call, err, "image_confusion")
    for c in (5, 1, 0, -2):
        assert call(C=c) == -1 and f"image_confusion: C must lie in [2, 4], got {c}" in err()
    assert call(weight=None) == -1 and "wcm goes with weight: both or neither, got wcm without weight" in err()
    assert call(wcm=None) == -1 and "got weight without wcm" in err()
    for kw in (dict(pred=None), dict(truth=None), dict(cm=None), dict(invalid=None)):
        assert call(**kw) == -1 and "image_confusion: null pointer" in err(), kw
    for kw in (dict(weight=18), dict(cm=20), dict(wcm=20), dict(invalid=12)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(N=0) == 0 and call(N=0, weight=None, wcm=None) == 0                     # nothing to do, nothing launched


def test_component_measure_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(labels=16, weight=16, xq=16, yq=16, N=1, H=8, W=8, cap=4, out=16):
        return lib.usseg_component_measure(labels, weight, xq, yq, N, H, W, cap, out, None)

    _shape_checks(call, err, "component_measure")
    for c in (-1, 65):
        assert call(cap=c) == -1 and f"component_measure: the cap must lie in [0, H*W], got {c}" in err()
    for kw in (dict(labels=None), dict(weight=None), dict(xq=None), dict(yq=None), dict(out=None)):
        assert call(**kw) == -1 and "component_measure: null pointer" in err(), kw
    for kw in (dict(labels=18), dict(weight=18), dict(xq=17), dict(yq=22), dict(out=20)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(N=0) == 0 and call(cap=0, out=None) == 0


def test_bootstrap_sums_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(rows=16, U=3, K=4, seed=1, R=2, out=16):
        return lib.usseg_bootstrap_sums(rows, U, K, seed, R, out, None)

    for k in (17, 0, -1):
        assert call(K=k) == -1 and f"bootstrap_sums: K must lie in [1, 16], got {k}" in err()
    assert call(U=0) == -1 and "bootstrap_sums: 2 replicates of an empty table (U = 0)" in err()
    for kw in (dict(U=-1), dict(U=(1 << 20) + 1)):
        assert call(**kw) == -1 and "bootstrap_sums: U must lie in [0, 2^20]" in err(), kw
    for kw in (dict(R=-1), dict(R=(1 << 20) + 1)):
        assert call(**kw) == -1 and "bootstrap_sums: R must lie in [0, 2^20]" in err(), kw
    for kw in (dict(out=None), dict(rows=None)):
        assert call(**kw) == -1 and "bootstrap_sums: null pointer" in err(), kw
    for kw in (dict(rows=20), dict(out=12)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(R=0) == 0 and call(R=0, out=None) == 0 and call(U=0, R=0, rows=None, out=None) == 0
    assert call(seed=2 ** 64 - 1, R=0) == 0


def test_the_wrappers_run_on_the_gpu_only_and_check_before_they_call():
    from ultrasound_modeling_amd import TBIEvaluator as E
    from ultrasound_modeling_amd import ops
    m = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(AssertionError, match="GPU"):
        ops.image_confusion(m, m)
    with pytest.raises(AssertionError, match="GPU"):
        ops.component_measure(torch.zeros((1, 4, 4), dtype=torch.int32), *[torch.zeros((4, 4), dtype=torch.int32)] * 3, 2)
    with pytest.raises(AssertionError, match="GPU"):
        ops.bootstrap_sums(torch.zeros((3, 2), dtype=torch.int64), 4)
    for fn, kwonly in ((ops.image_confusion, ("out",)), (ops.component_measure, ("out",)), (ops.bootstrap_sums, ("out", "check"))):
        par = inspect.signature(fn).parameters
        assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kwonly), fn
    assert ops.COMPONENT_MEASURE_FIELDS == ("pixels", "sum_w", "sum_wx", "sum_wy", "xq_min", "xq_max", "yq_min", "yq_max")
    par = inspect.signature(E.image_scores).parameters
    assert (par["geometry"].default, par["threshold"].default, par["pred_mask"].default) == (None, 0.5, None)
    src = inspect.getsource(E.main) + inspect.getsource(E._add_score_arguments)
    for flag in ("--scores-csv", "--patient-csv", "--lesion-size-csv", "--patient-regex", "--bootstrap", "--bootstrap-seed"):
        assert flag in src, flag


# ------------------------------------------------------------------------------------------------ the evaluator's writers and main
@pytest.fixture
def run(monkeypatch):
    """the synthetic run, its geometry, and the seven GPU wrappers replaced by the restatements (CPU tensors)"""
    from ultrasound_modeling_amd import TBIEvaluator as E
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.metrics import ScanGeometry
    for name, fn in SR.STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    res = SR.synthetic_result(E)
    X, Y = SR.polar_axes(*res.label.shape[1:])
    return types.SimpleNamespace(E=E, res=res, X=X, Y=Y, geo=ScanGeometry(X, Y), pred=res.bleed_prob > 0.5, true=res.label > 1.5)


def _floats(cells):
    return [float(c) if c != "" else None for c in cells]


def test_write_scores_csv_rows_by_hand(run, tmp_path):
    E, res, geo = run.E, run.res, run.geo
    path = tmp_path / "scores.csv"
    assert E.write_scores_csv(str(path), res, geo, device="cpu") == 6
    rows = list(csv.reader(open(path)))
    head = ["name", "tp", "fp", "fn", "tn", "dice", "iou", "sensitivity", "precision", "area_true", "area_pred", "area_tp", "area_dice", "area_error"]
    assert rows[0] == head and [r[0] for r in rows[1:]] == [str(n) for n in res.names] + ["pooled", "mean", "median", "defined", "loa_lower", "loa_upper"]
    # one data row by hand, from boolean sums (not from the confusion loop)
    p, t = run.pred[0], run.true[0]
    tp, fp, fn, tn = int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())
    assert tp > 0 and fp > 0 and fn > 0
    wt, wp, wtp = (int(geo.wq[m].astype(np.int64).sum()) for m in (t, p, p & t))
    want = [tp, fp, fn, tn, 2 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn), tp / (tp + fn), tp / (tp + fp), wt * geo.quantum, wp * geo.quantum, wtp * geo.quantum,
            2 * wtp / (wt + wp), (wp - wt) * geo.quantum]
    assert [int(c) for c in rows[1][1:5]] == want[:4] and _floats(rows[1][5:]) == want[4:]
    assert abs(want[8] - geo.area[t].sum()) <= int(t.sum()) * geo.quantum / 2 * (1 + 1e-9)          # the area is the area, to the documented bound
    # image 1 is empty in both masks: every ratio undefined; image 2 predicts nothing: Dice 0, precision undefined
    assert rows[2][1:5] == ["0", "0", "0", str(p.size)] and rows[2][5:9] == ["nan"] * 4 and rows[2][12] == "nan" and float(rows[2][13]) == 0.0
    assert float(rows[3][5]) == 0.0 and rows[3][8] == "nan" and float(rows[3][13]) < 0
    # the summary rows
    table = E.image_scores(res, geo, device="cpu")
    for c in ("tp", "fp", "fn", "tn"):
        assert int(rows[7][head.index(c)]) == int(table[c].sum()) == sum(int(r[head.index(c)]) for r in rows[1:7])
    TP, FP, FN = (int(table[c].sum()) for c in ("tp", "fp", "fn"))
    assert float(rows[7][5]) == 2 * TP / (2 * TP + FP + FN)
    dice = np.array([float(r[5]) for r in rows[1:7]])
    assert float(rows[8][5]) == np.nanmean(dice) and float(rows[9][5]) == np.nanmedian(dice) and rows[10][5] == "5" and rows[10][8] == "4"
    assert rows[8][1:5] == [""] * 4 and rows[11][1:13] == [""] * 12
    err = np.array([float(r[13]) for r in rows[1:7]])
    bias, sd = err.mean(), err.std(ddof=1)
    assert float(rows[8][13]) == bias and float(rows[11][13]) == bias - 1.96 * sd and float(rows[12][13]) == bias + 1.96 * sd
    # without a geometry: no area columns, no limits of agreement; the pixel columns are the same
    plain = tmp_path / "plain.csv"
    E.write_scores_csv(str(plain), res, device="cpu")
    prow = list(csv.reader(open(plain)))
    assert prow[0] == head[:9] and [r[:9] for r in rows[:11]] == prow and len(prow) == 11
    # pred_mask replaces the threshold rule; a threshold moves it
    E.write_scores_csv(str(plain), res, pred_mask=run.true, device="cpu")
    assert all(float(r[5]) == 1.0 for i, r in enumerate(list(csv.reader(open(plain)))[1:7]) if i != 1)
    assert E.image_scores(res, threshold=1.0, device="cpu")["tp"].sum() == 0 < E.image_scores(res, threshold=0.95, device="cpu")["tp"].sum() < table["tp"].sum()


def test_write_patient_csv_and_the_cluster_bootstrap(run, tmp_path):
    from ultrasound_modeling_amd import metrics as M
    E, res, geo = run.E, run.res, run.geo
    path = tmp_path / "patients.csv"
    assert E.write_patient_csv(str(path), res, geo, bootstrap=200, seed=11, device="cpu") == 3
    rows = list(csv.reader(open(path)))
    head = rows[0]
    assert head[:3] == ["patient", "n_images", "tp"] and head[3:] == list(E.SCORE_COLUMNS[1:]) + list(E.AREA_COLUMNS)
    assert [r[0] for r in rows[1:]] == ["001", "002", "003", "pooled", "mean", "median", "defined", "loa_lower", "loa_upper", "ci_pooled_lower",
                                        "ci_pooled_upper", "ci_mean_lower", "ci_mean_upper"]
    assert [r[1] for r in rows[1:5]] == ["2", "2", "2", "6"]
    t = E.image_scores(res, geo, device="cpu")
    for i in range(3):                                                                  # a patient's row: its two images' counts summed
        tp, fp, fn = (int(t[c][2 * i] + t[c][2 * i + 1]) for c in ("tp", "fp", "fn"))
        assert [int(rows[1 + i][head.index(c)]) for c in ("tp", "fp", "fn")] == [tp, fp, fn]
        assert float(rows[1 + i][head.index("dice")]) == 2 * tp / (2 * tp + fp + fn)
        assert float(rows[1 + i][head.index("area_error")]) == float((t["w_pred"][2 * i:2 * i + 2].sum() - t["w_true"][2 * i:2 * i + 2].sum()) * geo.quantum)
    pdice = [float(rows[1 + i][head.index("dice")]) for i in range(3)]
    assert float(rows[5][head.index("dice")]) == np.mean(pdice) and rows[7][head.index("dice")] == "3"
    # the intervals: the restatement's replicates of the PATIENT rows, the same host formulas
    groups = [M.patient_of(n) for n in res.names]
    names, prow = M.bootstrap_rows(t, groups)
    assert prow.shape == (3, 8) and prow[:, 0].tolist() == [int(t["tp"][2 * i] + t["tp"][2 * i + 1]) for i in range(3)]
    st = M.bootstrap_statistics(names, SR.bootstrap(prow, 200, 11), geo.quantum)
    ci = {k: tuple(np.quantile(v[~np.isnan(v)], [0.025, 0.975])) for k, v in st.items()}
    d, ad, ae = head.index("dice"), head.index("area_dice"), head.index("area_error")
    assert (float(rows[10][d]), float(rows[11][d])) == ci["pooled_dice"] and (float(rows[12][d]), float(rows[13][d])) == ci["mean_dice"]
    assert (float(rows[10][ad]), float(rows[11][ad])) == ci["area_dice"] and (float(rows[10][ae]), float(rows[11][ae])) == ci["area_error_total"]
    assert ci["pooled_dice"][0] <= float(rows[4][d]) <= ci["pooled_dice"][1] and ci["pooled_dice"][0] < ci["pooled_dice"][1]
    # another pattern: every image its own patient
    assert E.write_patient_csv(str(path), res, pattern=r"frame\d+", device="cpu") == 6
    assert [r[0] for r in list(csv.reader(open(path)))[1:7]] == [f"frame{i}" for i in range(6)]


def test_write_lesion_size_csv_rows(run, tmp_path):
    E, res, geo = run.E, run.res, run.geo
    path = tmp_path / "sizes.csv"
    n = E.write_lesion_size_csv(str(path), res, geo, min_area=3, device="cpu")
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["name", "kind", "id", "pixels", "area", "diameter", "centroid_x", "centroid_y", "x_min", "x_max", "y_min", "y_max", "matched"]
    cleaned = CR.clean(run.pred.astype(np.uint8), res.bleed_prob, 8, 3, 0.0)
    lp, cp = CR.label(cleaned, 8)
    lt, ct = CR.label(run.true.astype(np.uint8), 8)
    assert n == len(rows) - 1 == int(cp.sum() + ct.sum()) and cp.tolist() == [1, 0, 0, 1, 1, 1] and ct.tolist() == [1, 0, 1, 1, 1, 1]
    assert [(r[0], r[1], r[2]) for r in rows[1:4]] == [("DoD001_frame0", "pred", "1"), ("DoD001_frame0", "true", "1"), ("DoD002_frame2", "true", "1")]
    assert [r[12] for r in rows[1:4]] == ["1", "1", "0"]                               # image 2's lesion has no prediction to match
    # the first row by hand: the component's own pixels
    sel = lp[0] == 1
    w = geo.wq[sel].astype(np.int64)
    area = int(w.sum()) * geo.quantum
    want = [int(sel.sum()), area, 2.0 * math.sqrt(area / math.pi), geo.x_min + geo.xstep * (int((w * geo.xq[sel]).sum()) / int(w.sum())),
            geo.y_min + geo.ystep * (int((w * geo.yq[sel]).sum()) / int(w.sum())), geo.x_min + geo.xstep * int(geo.xq[sel].min()),
            geo.x_min + geo.xstep * int(geo.xq[sel].max()), geo.y_min + geo.ystep * int(geo.yq[sel].min()), geo.y_min + geo.ystep * int(geo.yq[sel].max())]
    assert int(rows[1][3]) == want[0] and _floats(rows[1][4:12]) == want[1:]
    assert abs(want[1] - geo.area[sel].sum()) <= want[0] * geo.quantum / 2 * (1 + 1e-9)
    assert abs(want[3] - (w * run.X[sel]).sum() / w.sum()) <= geo.xstep / 2 * (1 + 1e-9) and run.X[sel].min() - geo.xstep <= want[5] <= want[3] <= want[6]
    # without the clean-up the speckle shows as components of its own
    assert E.write_lesion_size_csv(str(path), res, geo, device="cpu") > n
    from ultrasound_modeling_amd import metrics as M
    s = M.lesion_sizes(cleaned, geo, device="cpu")
    assert s["count"].tolist() == cp.tolist() and s["pixels"].shape == (6, 1) and s["area"][0, 0] == want[1] and np.isnan(s["area"][1, 0])
    assert s["pixels"][1, 0] == 0 and np.isnan(s["x_min"][2, 0]) and s["diameter"][0, 0] == want[2]


def test_write_lesion_csv_is_what_it_was(run, tmp_path):
    """the existing lesion table of the same run, restated from its documented format: the new columns live in files of their own"""
    E, res = run.E, run.res
    path = tmp_path / "lesion.csv"
    assert E.write_lesion_csv(str(path), res, min_area=3, device="cpu") == 6
    s = CR.lesion_scores(CR.clean(run.pred.astype(np.uint8), res.bleed_prob, 8, 3, 0.0), run.true, 8)
    cols = ("n_true", "n_pred", "detected", "missed", "false_pos", "largest_true", "largest_pred")
    lines = ["name," + ",".join(cols) + ",sensitivity,precision,f1,fp_per_image"]
    lines += [",".join([str(n)] + [str(int(s[c][i])) for c in cols] + [""] * 4) for i, n in enumerate(res.names)]
    lines.append(",".join(["total"] + [str(int(s[c].max() if c.startswith("largest") else s[c].sum())) for c in cols]
                          + [repr(float(s[k])) for k in ("sensitivity", "precision", "f1", "fp_per_image")]))
    assert open(path, newline="").read() == "\r\n".join(lines) + "\r\n"
    assert E.LESION_COLUMNS == cols


def test_mains_flags(run, tmp_path, monkeypatch, capsys):
    E, res = run.E, run.res
    monkeypatch.setattr(E.Cascade, "from_checkpoints", classmethod(lambda cls, *a, **k: types.SimpleNamespace(device=torch.device("cpu"))))
    monkeypatch.setattr(E.ConeGeometry, "from_dir", classmethod(lambda cls, *a, **k: None))
    monkeypatch.setattr(E, "Polar_Model", lambda data, cascade, names=None, batch_size=16: res)
    monkeypatch.setattr(E, "Display", lambda *a, **k: [])
    axis = tmp_path / "axis"
    axis.mkdir()
    np.save(axis / "xAxis.npy", run.X)
    np.save(axis / "yAxis.npy", run.Y)
    np.save(tmp_path / "data.npy", np.zeros((6, 1, 1, 1, 12)))
    np.save(tmp_path / "paths.npy", res.names)
    base = [str(tmp_path / "data.npy"), str(tmp_path / "paths.npy"), str(axis), str(tmp_path / "out"), "--bleed", "none.pt"]
    sc, pc, lc, les = (tmp_path / n for n in ("s.csv", "p.csv", "l.csv", "lesion.csv"))
    E.main(base + ["--scores-csv", str(sc), "--patient-csv", str(pc), "--lesion-size-csv", str(lc), "--lesion-csv", str(les), "--bootstrap", "50",
                   "--bootstrap-seed", "7", "--min-area", "3", "--threshold", "0.4"])
    out = capsys.readouterr().out
    assert "wrote 6 image-score rows" in out and "wrote 3 patient rows" in out and "lesion-size rows" in out and "wrote 6 lesion rows" in out
    # what main wrote is what the writers write for the same settings: the UNCAST axes, the cleaned prediction, the threshold, the seed
    geo = run.geo
    cleaned = E.clean_result(res, 0.4, min_area=3, min_peak=0.0, connectivity=8, device="cpu")
    assert np.array_equal(cleaned, CR.clean((res.bleed_prob > 0.4).astype(np.uint8), res.bleed_prob, 8, 3, 0.0)) and cleaned.sum() < (res.bleed_prob > 0.4).sum()
    E.write_scores_csv(str(tmp_path / "s2.csv"), res, geo, pred_mask=cleaned, bootstrap=50, seed=7, device="cpu")
    E.write_patient_csv(str(tmp_path / "p2.csv"), res, geo, pred_mask=cleaned, bootstrap=50, seed=7, device="cpu")
    E.write_lesion_size_csv(str(tmp_path / "l2.csv"), res, geo, 0.4, min_area=3, device="cpu")
    E.write_lesion_csv(str(tmp_path / "lesion2.csv"), res, 0.4, min_area=3, device="cpu")
    for a, b in ((sc, "s2.csv"), (pc, "p2.csv"), (lc, "l2.csv"), (les, "lesion2.csv")):
        assert open(a).read() == open(tmp_path / b).read(), b
    srows = list(csv.reader(open(sc)))
    assert [r[0] for r in srows[-4:]] == ["ci_pooled_lower", "ci_pooled_upper", "ci_mean_lower", "ci_mean_upper"]
    assert float(srows[-4][5]) <= float(srows[7][5]) <= float(srows[-3][5])
    # --patient-regex
    E.main(base + ["--patient-csv", str(pc), "--patient-regex", r"frame(\d)"])
    assert [r[0] for r in list(csv.reader(open(pc)))[1:7]] == list("012345")
    capsys.readouterr()
    # without the new flags nothing of this runs: the geometry is not even read
    from ultrasound_modeling_amd import metrics as M

    def boom(*a, **k):
        raise AssertionError("not without the flags")
    monkeypatch.setattr(M.ScanGeometry, "from_dir", classmethod(boom))
    for name in ("image_confusion", "component_measure", "bootstrap_sums"):
        monkeypatch.setattr(E.ops, name, boom)
    os.remove(sc)
    E.main(base + ["--lesion-csv", str(les)])
    assert "image-score" not in capsys.readouterr().out and not sc.exists() and open(les).read() != open(tmp_path / "lesion2.csv").read()
    for bad in (["--bootstrap", "10"], ["--bootstrap", "-1", "--scores-csv", str(sc)], ["--scores-csv", str(sc), "--patient-regex", "("],
                ["--scores-csv", str(sc), "--bootstrap", str((1 << 20) + 1)], ["--scores-csv", str(sc), "--bootstrap-seed", "-1"]):
        with pytest.raises(SystemExit):
            E.main(base + bad)
