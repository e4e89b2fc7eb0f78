"""Connected components without a GPU: the flood-fill restatement (tests/components_restatement.py) against scipy.ndimage.label and against
hand answers, the score formulas on hand tables, and the C ABI - exported symbols, header text, workspace sizes and every argument check of
the four entry points before any launch."""
import inspect
import os

import numpy as np
import pytest

import components_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}
CASES = CR.label_cases()


# ------------------------------------------------------------------------------------------------ the restatement against SciPy
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_equals_scipys_labels_element_for_element(name, connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    mask = CASES[name]
    labels, count = CR.label(mask, connectivity)
    assert labels.dtype == np.int32 and labels.shape == mask.shape
    for n in range(mask.shape[0]):
        want, k = nd.label(mask[n], structure=STRUCTURE[connectivity])
        assert count[n] == k and np.array_equal(labels[n], want), (name, n)


def test_the_planted_shapes_are_what_they_claim():
    for c in (4, 8):
        assert CR.label(CR.spiral(33), c)[1].tolist() == [1]
        assert CR.label(CR.comb(), c)[1].tolist() == [1, 1]
    assert CR.spiral(33).sum() > 33 * 33 // 2
    assert CR.label(CR.checkerboard(16), 4)[1].tolist() == [128] and CR.label(CR.checkerboard(16), 8)[1].tolist() == [1]
    mixed = CASES["empty, random, full"]
    assert not mixed[0].any() and mixed[2].all() and not mixed[4].any()


# ------------------------------------------------------------------------------------------------ hand answers
HAND = np.array([[1, 1, 0, 0, 0, 1, 0],
                 [0, 0, 0, 1, 0, 1, 0],
                 [0, 0, 1, 0, 0, 0, 0],
                 [1, 0, 0, 0, 0, 1, 1],
                 [1, 0, 0, 0, 0, 1, 1]], np.uint8)


def test_a_5x7_mask_by_hand():
    l4, k4 = CR.label_plane(HAND, 4)
    assert k4 == 6
    assert l4.tolist() == [[1, 1, 0, 0, 0, 2, 0],
                           [0, 0, 0, 3, 0, 2, 0],
                           [0, 0, 4, 0, 0, 0, 0],
                           [5, 0, 0, 0, 0, 6, 6],
                           [5, 0, 0, 0, 0, 6, 6]]
    l8, k8 = CR.label_plane(HAND, 8)
    assert k8 == 5                                                # the diagonal pair (1,3) - (2,2) is one component at 8, two at 4
    assert l8.tolist() == [[1, 1, 0, 0, 0, 2, 0],
                           [0, 0, 0, 3, 0, 2, 0],
                           [0, 0, 3, 0, 0, 0, 0],
                           [4, 0, 0, 0, 0, 5, 5],
                           [4, 0, 0, 0, 0, 5, 5]]
    prob = np.full((1, 5, 7), 0.25, np.float32)
    prob[0, 2, 2] = 0.75
    prob[0, 1, 3] = np.nan
    st = CR.stats(l8[None], 6, prob)
    bits = lambda v: int(np.float32(v).view(np.uint32))
    assert st[0, 0].tolist() == [2, 0, 0, 0, 1, 0, 1, bits(0.25)]
    assert st[0, 2].tolist() == [2, 1, 2, 2, 3, 3, 5, bits(0.75)]  # the NaN at (1,3) does not win
    assert st[0, 4].tolist() == [4, 3, 5, 4, 6, 14, 22, bits(0.25)]
    assert not st[0, 5].any()                                     # id 6 does not exist at 8
    assert CR.stats(l8[None], 2, None)[0].tolist() == [[2, 0, 0, 0, 1, 0, 1, 0], [2, 0, 5, 1, 5, 1, 10, 0]]
    assert CR.clean(HAND[None], None, 8, min_area=3)[0].tolist() == (l8 == 5).astype(int).tolist()
    assert CR.clean(HAND[None], None, 4, min_area=2)[0].tolist() == ((l4 > 0) & (l4 != 3) & (l4 != 4)).astype(int).tolist()
    assert CR.clean(HAND[None], prob, 8, min_area=1, min_peak=0.5)[0].tolist() == (l8 == 3).astype(int).tolist()
    assert CR.clean(HAND[None], None, 8, min_area=1)[0].tolist() == HAND.tolist()
    other = np.zeros((5, 7), np.uint8)
    other[0:2, 1:6] = 1                                           # one component that touches ids 1, 2 and 3 of l8
    lo, ko = CR.label_plane(other, 8)
    ha, hb = CR.overlap(l8[None], lo[None], 5, 1)
    assert ko == 1 and ha.tolist() == [[1, 2, 1, 0, 0]] and hb.tolist() == [[4]]


def test_lesion_scores_from_tables_by_hand():
    from ultrasound_modeling_amd.metrics import lesion_scores_from_tables
    # image 0: 2 lesions, 3 predicted; image 1: no lesion, 1 predicted; image 2: 1 lesion, nothing predicted; image 3: nothing at all
    count_t, count_p = [2, 0, 1, 0], [3, 1, 0, 0]
    hit_t = [[5, 1], [9, 9], [0, 7], [0, 0]]                      # (columns past the count hold rubbish on purpose)
    hit_p = [[4, 0, 2], [0, 3, 3], [8, 8, 8], [0, 0, 0]]
    area_t = [[9, 4], [50, 50], [6, 99], [0, 0]]
    area_p = [[7, 1, 3], [2, 77, 77], [9, 9, 9], [0, 0, 0]]
    s = lesion_scores_from_tables(count_t, count_p, hit_t, hit_p, area_t, area_p)
    assert s["n_true"].tolist() == count_t and s["n_pred"].tolist() == count_p
    assert s["detected"].tolist() == [2, 0, 0, 0] and s["missed"].tolist() == [0, 0, 1, 0] and s["false_pos"].tolist() == [1, 1, 0, 0]
    assert s["largest_true"].tolist() == [9, 0, 6, 0] and s["largest_pred"].tolist() == [7, 2, 0, 0]
    assert s["sensitivity"] == 2 / 3 and s["precision"] == 2 / 4 and s["fp_per_image"] == 2 / 4
    assert s["f1"] == 2 * 0.5 * (2 / 3) / (0.5 + 2 / 3)
    s2 = lesion_scores_from_tables(count_t, count_p, hit_t, hit_p, area_t, area_p, min_overlap=2)
    assert s2["detected"].tolist() == [1, 0, 0, 0] and s2["missed"].tolist() == [1, 0, 1, 0] and s2["sensitivity"] == 1 / 3
    # div_no_nan: no lesion and no prediction anywhere
    e = lesion_scores_from_tables([0, 0], [0, 0], np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)))
    assert (e["sensitivity"], e["precision"], e["f1"], e["fp_per_image"]) == (0.0, 0.0, 0.0, 0.0) and e["largest_true"].tolist() == [0, 0]
    z = lesion_scores_from_tables([], [], np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)))
    assert z["fp_per_image"] == 0.0 and z["n_true"].shape == (0,)
    # lesions without a prediction: sensitivity 0, precision div_no_nan
    m = lesion_scores_from_tables([2], [0], [[0, 0]], np.zeros((1, 0)), [[3, 4]], np.zeros((1, 0)))
    assert m["missed"].tolist() == [2] and m["sensitivity"] == 0.0 and m["precision"] == 0.0 and m["f1"] == 0.0
    with pytest.raises(ValueError):
        lesion_scores_from_tables([2], [0], [[1]], np.zeros((1, 0)), [[3, 4]], np.zeros((1, 0)))
    with pytest.raises(ValueError):
        lesion_scores_from_tables(count_t, count_p, hit_t, hit_p, area_t, area_p, min_overlap=0)


def test_the_restatements_scores_equal_the_table_formulas():
    from ultrasound_modeling_amd.metrics import lesion_scores_from_tables
    pred, true = CR.random_mask((3, 12, 14), 0.3, 7), CR.random_mask((3, 12, 14), 0.25, 8)
    pred[2] = 0
    for c, mo in ((4, 1), (8, 1), (8, 2)):
        lp, cp = CR.label(pred, c)
        lt, ct = CR.label(true, c)
        cap_t, cap_p = int(ct.max()), int(cp.max())
        hit_t, hit_p = CR.overlap(lt, lp, cap_t, cap_p)
        got = lesion_scores_from_tables(ct, cp, hit_t, hit_p, CR.stats(lt, cap_t)[..., 0], CR.stats(lp, cap_p)[..., 0], mo)
        want = CR.lesion_scores(pred, true, c, mo)
        for k, v in want.items():
            assert np.array_equal(got[k], v), (c, mo, k)


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


NEW_SYMBOLS = ("usseg_components_ws_bytes", "usseg_label_components", "usseg_component_stats", "usseg_clean_mask", "usseg_component_overlap")


def test_exported_symbols_header_text_and_build():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in hdr, name
    for text in ("scipy.ndimage.label's numbering", "area, y_min, x_min, y_max, x_max, sum of y, sum of x, peak", "out may alias mask",
                 "a NaN never wins", "Ids above the caps are skipped", "one\n * linear chain"):
        assert text in hdr, text
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    assert mk.count("components.hip") == 2                           # built, and with the packed-fp32 flags off like its neighbours
    from ultrasound_modeling_amd import TBIEvaluator, metrics, ops
    for fn in ("components_ws_bytes", "label_components", "component_stats", "clean_mask", "component_overlap"):
        assert callable(getattr(ops, fn)), fn
    assert inspect.signature(ops.label_components).parameters["connectivity"].default == 8
    par = inspect.signature(ops.clean_mask).parameters
    assert (par["connectivity"].default, par["min_area"].default, par["min_peak"].default) == (8, 1, 0.0)
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("connectivity", "min_area", "min_peak", "out", "ws"))
    assert callable(metrics.components) and callable(metrics.lesion_scores)
    assert TBIEvaluator.PolarResult._fields == ("prob_map", "bleed_prob", "mask", "label", "bmode", "names")
    assert TBIEvaluator.CascadeOutput._fields == ("probs", "mask", "prob_map", "bleed_prob")
    par = inspect.signature(TBIEvaluator.clean_result).parameters
    assert par["min_area"].default is inspect.Parameter.empty and par["min_area"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (TBIEvaluator.surface_scores, TBIEvaluator.write_surface_csv):
        p = inspect.signature(fn).parameters["pred_mask"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    src = inspect.getsource(TBIEvaluator.main)
    for flag in ("--lesion-csv", "--min-area", "--min-peak", "--connectivity"):
        assert flag in src, flag


def test_workspace_sizes():
    L, lib = _lib()
    assert lib.usseg_components_ws_bytes(16, 256, 80) == 3 * 4 * 16 * 256 * 80 + 4 * 16 * 256
    assert lib.usseg_components_ws_bytes(3, 5, 7) == 3 * 432 + 64                 # each region rounded up to 16 bytes
    assert lib.usseg_components_ws_bytes(0, 5, 7) == 0
    assert lib.usseg_components_ws_bytes(8, 8192, 8192) == 3 * 4 * (1 << 29) + 4 * 8 * 8192
    for bad in ((1, 0, 8), (1, 8, 0), (1, 8193, 8), (1, 8, 8193), (-1, 8, 8), (65536, 1, 1), (9, 8192, 8192)):
        assert lib.usseg_components_ws_bytes(*bad) == -1, bad
    from ultrasound_modeling_amd import ops
    assert ops.components_ws_bytes(2, 67, 129) == lib.usseg_components_ws_bytes(2, 67, 129)
    with pytest.raises(ValueError):
        ops.components_ws_bytes(1, 8193, 8)


def _shape_checks(call, err, what):
    for kw in (dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(H=-3)):
        assert call(**kw) == -1 and f"{what}: H and W must lie in [1, 8192]" in err(), kw
    for n in (-1, 65536):
        assert call(N=n) == -1 and f"{what}: 0 <= N <= 65535" in err()
    assert call(N=9, H=8192, W=8192) == -1 and f"{what}: more than 2^29 pixels" in err()


def test_label_components_refuses_bad_arguments_before_any_launch():
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(mask=16, N=1, H=8, W=8, conn=8, labels=16, count=16, ws=16, ws_bytes=1 << 40):
        return lib.usseg_label_components(mask, N, H, W, conn, labels, count, ws, ws_bytes, None)

    _shape_checks(call, err, "label_components")
    for c in (6, 0, -8, 2):
        assert call(conn=c) == -1 and f"label_components: connectivity must be 4 or 8, got {c}" in err()
    for kw in (dict(mask=None), dict(labels=None), dict(count=None), dict(ws=None)):
        assert call(**kw) == -1 and "label_components: null pointer" in err(), kw
    for kw in (dict(labels=18), dict(count=17), dict(ws=24)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    need = lib.usseg_components_ws_bytes(1, 8, 8)
    assert need == 3 * 256 + 32
    assert call(ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    assert call(N=0) == 0                                                         # nothing to do, nothing launched


def test_component_stats_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(labels=16, prob=16, N=1, H=8, W=8, cap=4, stats=16):
        return lib.usseg_component_stats(labels, prob, N, H, W, cap, stats, None)

    _shape_checks(call, err, "component_stats")
    for c in (-1, 65):
        assert call(cap=c) == -1 and f"component_stats: the cap must lie in [0, H*W], got {c}" in err()
    for kw in (dict(labels=None), dict(stats=None)):
        assert call(**kw) == -1 and "component_stats: null pointer" in err(), kw
    for kw in (dict(labels=18), dict(prob=18), dict(stats=20)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(N=0) == 0 and call(N=0, prob=None) == 0 and call(cap=0, stats=None) == 0


def test_clean_mask_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(mask=16, prob=16, N=1, H=8, W=8, conn=8, min_area=2, min_peak=0.5, out=16, ws=16, ws_bytes=1 << 40):
        return lib.usseg_clean_mask(mask, prob, N, H, W, conn, min_area, min_peak, out, ws, ws_bytes, None)

    _shape_checks(call, err, "clean_mask")
    for c in (6, 0):
        assert call(conn=c) == -1 and f"clean_mask: connectivity must be 4 or 8, got {c}" in err()
    assert call(min_peak=float("nan")) == -1 and "clean_mask: min_peak is NaN" in err()
    for kw in (dict(mask=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -1 and "clean_mask: null pointer" in err(), kw
    for kw in (dict(prob=18), dict(ws=8)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    need = lib.usseg_components_ws_bytes(1, 8, 8)
    assert call(ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    assert call(min_area=1, min_peak=0.0, ws_bytes=0) == -1 and "the workspace holds 0 bytes" in err()      # the copy path checks it all the same
    assert call(N=0) == 0 and call(N=0, prob=None) == 0


def test_component_overlap_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(la=16, lb=16, N=1, H=8, W=8, cap_a=4, cap_b=4, hit_a=16, hit_b=16):
        return lib.usseg_component_overlap(la, lb, N, H, W, cap_a, cap_b, hit_a, hit_b, None)

    _shape_checks(call, err, "component_overlap")
    for kw in (dict(cap_a=-1), dict(cap_b=-1), dict(cap_a=65), dict(cap_b=65)):
        assert call(**kw) == -1 and "component_overlap: the caps must lie in [0, H*W]" in err(), kw
    for kw in (dict(la=None), dict(lb=None), dict(hit_a=None), dict(hit_b=None)):
        assert call(**kw) == -1 and "component_overlap: null pointer" in err(), kw
    for kw in (dict(la=18), dict(lb=18), dict(hit_a=18), dict(hit_b=17)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(N=0) == 0 and call(cap_a=0, cap_b=0, hit_a=None, hit_b=None) == 0
