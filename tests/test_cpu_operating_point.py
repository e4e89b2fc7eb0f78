"""Threshold sweeps and temperature scaling without a GPU: ``metrics.sweep_from_counts`` against a brute-force count over every pixel pair and
every threshold, hand-computed known answers that pin the NumPy restatement (tests/operating_point_restatement.py) the device tests compare the
kernels with, the bracket search against a dense fp64 search, every argument check of csrc/operating_point.hip (an error code and a message
before any launch), the refusals of the Python surface and the three new symbols."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import operating_point_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("usseg_score_sweep", "usseg_temperature_nll", "usseg_apply_temperature")


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the sweep's host arithmetic
@pytest.mark.parametrize("cls", [0, 2])
def test_sweep_from_counts_against_a_brute_force_count(cls):
    from ultrasound_modeling_amd.metrics import sweep_from_counts, sweep_line
    rng = np.random.default_rng(3)
    bins = 16
    probs = _softmax(2 * rng.standard_normal((2, 5, 7, 3)))
    y = np.eye(3, dtype=np.float32)[rng.integers(0, 3, (2, 5, 7))]
    flat = probs.reshape(-1, 3)
    flat[0] = (0.0, 0.0, 1.0)
    flat[1] = (1.0, 0.0, 0.0)
    flat[2] = (0.25, 0.25, 0.5)                         # on bin edges
    flat[3] = np.nan                                    # invalid
    counts = R.sweep_counts(probs, y, bins, cls)
    got = sweep_from_counts(counts)
    b, valid = R.sweep_bins(flat[:, cls], bins)
    pos = (R.first_max(y.reshape(-1, 3)) == cls)
    b, pos = b[valid], pos[valid]
    assert got["n_invalid"] == 1 and len(b) == 69
    for k in range(bins + 1):
        pred = b >= k
        tp, fp, fn, tn = int((pred & pos).sum()), int((pred & ~pos).sum()), int((~pred & pos).sum()), int((~pred & ~pos).sum())
        assert (got["tp"][k], got["fp"][k], got["fn"][k], got["tn"][k]) == (tp, fp, fn, tn), k
        assert got["tpr"][k] == tp / pos.sum() and got["fpr"][k] == fp / (~pos).sum()
        assert got["precision"][k] == (tp / (tp + fp) if tp + fp else 1.0)
        assert got["dice"][k] == (2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    # every (positive, negative) pair: the positive ranks higher = 1, a tie = 1/2
    wins2 = sum(2 * int(bp > bn) + int(bp == bn) for bp in b[pos] for bn in b[~pos])
    assert got["auc"] == wins2 / (2 * int(pos.sum()) * int((~pos).sum())) and 0.0 < got["auc"] < 1.0
    P = int(pos.sum())
    ap = sum((got["tp"][k] - got["tp"][k + 1]) / P * got["precision"][k] for k in range(bins))
    assert abs(got["average_precision"] - ap) <= 1e-15
    kd = int(np.argmax(got["dice"]))                    # argmax: the first (smallest) k of the maximum
    assert got["best_dice"] == (kd, float(got["threshold"][kd]), float(got["dice"][kd]))
    ky = int(np.argmax(got["tpr"] - got["fpr"]))
    assert got["best_youden"][0] == ky and got["best_youden"][2] == float(got["tpr"][ky] - got["fpr"][ky])
    # the pure-Python restatement agrees key by key
    want = R.sweep_from_counts(counts)
    for key in ("tp", "fp", "fn", "tn", "tpr", "fpr", "precision", "dice", "threshold"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key
    for key in ("auc", "average_precision", "best_dice", "best_youden", "n_invalid"):
        assert got[key] == want[key], key
    assert "AUC = {:.5f}".format(got["auc"]) in sweep_line(got) and "best Dice" in sweep_line(got)


def test_sweep_known_answers():
    from ultrasound_modeling_amd.metrics import sweep_from_counts
    # bins = 2: bin 0 holds 3 negatives and 1 positive, bin 1 holds 1 negative and 3 positives, 2 invalid
    r = sweep_from_counts(np.array([3, 1, 1, 3, 2]))
    assert r["tp"].tolist() == [4, 3, 0] and r["fp"].tolist() == [4, 1, 0] and r["fn"].tolist() == [0, 1, 4] and r["tn"].tolist() == [0, 3, 4]
    assert r["tpr"].tolist() == [1.0, 0.75, 0.0] and r["fpr"].tolist() == [1.0, 0.25, 0.0]
    assert r["precision"].tolist() == [0.5, 0.75, 1.0] and r["dice"].tolist() == [8 / 12, 6 / 8, 0.0]
    # pairs: pos in bin 1 (3) beat neg in bin 0 (3) = 9, tie with neg in bin 1 = 1.5; pos in bin 0 (1) ties with 3 = 1.5, loses to 1: 12/16
    assert r["auc"] == 0.75
    assert r["average_precision"] == (4 - 3) / 4 * 0.5 + 3 / 4 * 0.75
    assert r["best_dice"] == (1, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.75) and r["best_youden"][0] == 1 and r["best_youden"][2] == 0.5
    assert r["n_invalid"] == 2 and r["threshold"][0] == -np.inf and r["threshold"][2] == 1.0
    none = sweep_from_counts(np.array([5, 0, 2, 0, 0]))                  # no positive: AUC, AP and the rates are NaN, precision 1, Dice 0
    assert math.isnan(none["auc"]) and math.isnan(none["average_precision"]) and np.isnan(none["tpr"]).all()
    assert none["precision"].tolist() == [0.0, 0.0, 1.0] and none["dice"].tolist() == [0.0, 0.0, 0.0] and none["best_dice"][0] == 0
    tie = sweep_from_counts(np.array([0, 2, 0, 0, 0, 0, 0, 0, 0]))      # only positives in bin 0: Dice is 1 at k = 0 alone
    assert tie["best_dice"][0] == 0 and tie["best_dice"][2] == 1.0
    with pytest.raises(ValueError):
        sweep_from_counts(np.zeros(7, np.int64))                        # bins = 3: not a power of two
    with pytest.raises(ValueError):
        sweep_from_counts(np.zeros(8, np.int64))


@pytest.mark.parametrize("bins", [2, 64, 4096])
def test_thresholds_turn_bin_at_least_k_into_a_strict_comparison(bins):
    from ultrasound_modeling_amd.metrics import sweep_thresholds
    thr = sweep_thresholds(bins)
    assert np.array_equal(thr, R.thresholds(bins)) and thr.dtype == np.float32 and len(thr) == bins + 1
    assert thr[0] == -np.inf and thr[bins] == 1.0
    for k in range(1, bins):
        assert thr[k] < np.float32(k / bins) and np.nextafter(thr[k], np.float32(1)) == np.float32(k / bins)
    edges = (np.arange(bins + 1) / bins).astype(np.float32)              # s exactly k/bins (0 and 1 included) and one ulp either side
    s = np.unique(np.clip(np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2)),
                                          np.array([0.0, 0.25, 0.5, 1.0, 0.3, 0.7], np.float32)]), 0, 1).astype(np.float32))
    b, valid = R.sweep_bins(s, bins)
    assert valid.all() and b[s == 1.0][0] == bins - 1 and b[s == 0.0][0] == 0
    ks = range(bins + 1) if bins <= 64 else list(range(0, bins + 1, 97)) + [1, bins - 1, bins]
    for k in ks:
        assert np.array_equal(b >= k, s > thr[k]), k


def test_sweep_counts_of_a_hand_made_input():
    probs = np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.0], [np.nan, 0.5], [0.1, 1.5], [0.2, -0.1], [0.0, 1.0]], np.float32).reshape(1, 1, 7, 2)
    y = np.array([[0, 1], [0, 1], [1, 0], [0, 1], [0, 1], [1, 0], [0.5, 0.5]], np.float32).reshape(1, 1, 7, 2)
    # class 1 scores: 0.5 (+) bin 2, 0.75 (+) bin 3, 0.0 (-) bin 0, 0.5 (+) bin 2, 1.5 invalid, -0.1 invalid, 1.0 (soft tie: label 0, -) bin 3
    assert R.sweep_counts(probs, y, 4, 1).tolist() == [1, 0, 0, 0, 0, 2, 1, 1, 2]
    # class 0 scores: 0.5 (-) bin 2, 0.25 (-) bin 1, 1.0 (+) bin 3, NaN invalid, 0.1 (-) bin 0, 0.2 (+) bin 0, 0.0 (+) bin 0
    assert R.sweep_counts(probs, y, 4, 0).tolist() == [1, 2, 1, 0, 1, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ the temperature
def test_nll_and_apply_known_answers():
    p = np.array([[0.5, 0.25, 0.25]], np.float32).reshape(1, 1, 1, 3)
    y = np.array([[0, 1, 0]], np.float32).reshape(1, 1, 1, 3)
    v, T, n, bad = R.nll(p, y, [1.0, 2.0])
    e = 1e-7                                                            # float32(1e-7) differs from 1e-7 by 1e-15: far below the tolerance
    z = np.log(np.array([0.5 + e, 0.25 + e, 0.25 + e]))
    for j, beta in enumerate((1.0, 2.0)):
        assert abs(v[0, j] - (np.log(np.exp(beta * z).sum()) - beta * z[1])) < 1e-13
        assert abs(T[0, j] - beta * abs(z[1])) < 1e-13
    assert abs(v[0, 0] - math.log(1 / 0.25)) < 1e-6 and abs(v[0, 1] - math.log(0.375 / 0.0625)) < 1e-6 and (n, bad) == (1, 0)
    out = R.apply_temperature(p, 2.0)
    assert np.allclose(out[0, 0, 0], np.array([0.25, 0.0625, 0.0625]) / 0.375, rtol=0, atol=1e-6)
    assert np.allclose(R.apply_temperature(p, 1.0), p, rtol=0, atol=1e-6)
    q = np.array([[0.5, np.nan, 0.5], [1.0, 0.0, 0.0]], np.float32).reshape(1, 1, 2, 3)
    o = R.apply_temperature(q, 0.5)
    assert np.isnan(o[0, 0, 0]).all() and abs(o[0, 0, 1].sum() - 1) < 1e-15 and o[0, 0, 1, 0] > 0.99
    # an invalid pixel contributes nothing and is counted; the quantised sum is the rounded fp64 sum here (one pixel, exact powers of two)
    pq = np.array([[0.5, 0.5], [0.5, np.nan], [1.5, 0.0]], np.float32).reshape(1, 1, 3, 2)
    yq = np.array([[1, 0]] * 3, np.float32).reshape(1, 1, 3, 2)
    c = R.nll_counts_f32(pq, yq, [1.0])
    assert c[1:] == [1, 2] and abs(c[0] - math.log(2) * 2 ** 20) <= 2
    assert R.nll_pixel_bound(10.0, 1.0, 3, 1, 1) > 0.5


@pytest.mark.parametrize("factor", [0.5, 1.0, 2.5])
def test_the_search_lands_within_one_final_spacing_of_a_dense_fp64_search(factor):
    """Probabilities whose logits were multiplied by ``factor`` against labels drawn from the un-multiplied ones: the fitted beta undoes it (about
    1 / factor); 96 pixels, 3 classes, all minimisers interior to [1/8, 8]."""
    from ultrasound_modeling_amd.metrics import temperature_candidates, temperature_search
    rng = np.random.default_rng(7)
    z = 2 * rng.standard_normal((1, 8, 12, 3))
    true = _softmax(z).astype(np.float64)
    true /= true.sum(-1, keepdims=True)
    lab = np.array([rng.choice(3, p=p) for p in true.reshape(-1, 3)]).reshape(1, 8, 12)
    y = np.eye(3, dtype=np.float32)[lab]
    probs = _softmax(factor * z)
    calls = []

    def evaluate(betas):
        calls.append(list(betas))
        return R.nll_counts_f32(probs, y, betas)
    beta, best, at1, spacing = R.search(evaluate)
    dense = R.dense_search(probs, y)
    print(f"factor {factor}: beta {beta:.5f}, dense {dense:.5f}, final spacing {spacing:.2e}")
    assert 1 / 8 < dense < 8 and abs(beta - dense) <= spacing and best <= at1
    assert abs(beta - 1 / factor) < 0.6 / factor                        # 96 pixels: the estimate is noisy, the direction is not
    # the product's search is the restated one: the same candidates, the same answer
    seen = list(calls)
    del calls[:]
    got = temperature_search(evaluate)
    assert calls == seen and got[0] == beta and got[1] == best and got[2] == at1 and got[4:] == (96, 0)
    assert got[3][0] <= beta <= got[3][1] or beta == 1.0
    assert temperature_candidates(1 / 8, 8.0, 16, True) == R.candidates(1 / 8, 8.0, 16, True)
    assert len(seen) == 5 and seen[-1] == [1.0] and all(len(b) == 16 for b in seen[:4])
    assert seen[0][0] == 0.125 and seen[0][-1] == 8.0 and all(b == float(np.float32(b)) for bs in seen for b in bs)


def test_the_search_names_the_edge_and_breaks_ties_to_the_smallest_beta():
    from ultrasound_modeling_amd.metrics import temperature_search
    with pytest.raises(ValueError, match="lower edge"):
        temperature_search(lambda b: [int(1000 * v) for v in b] + [1, 0])
    with pytest.raises(ValueError, match="upper edge"):
        temperature_search(lambda b: [int(-1000 * v) for v in b] + [1, 0])
    flat = temperature_search(lambda b: [5 if 0.5 < v < 3 else 9 for v in b] + [1, 0], rounds=1)
    assert flat[0] == min(v for v in R.candidates(1 / 8, 8.0, 16, True) if 0.5 < v < 3) and flat[1] == 5
    for bad in (dict(lo=0.0), dict(hi=17.0), dict(lo=2.0, hi=1.0), dict(candidates=17), dict(candidates=2), dict(rounds=0)):
        with pytest.raises(ValueError):
            temperature_search(lambda b: [0] * (len(b) + 2), **bad)


# ------------------------------------------------------------------------------------------------ symbols
def test_the_three_symbols_are_declared_listed_and_exported():
    from ultrasound_modeling_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert "#define USSEG_SWEEP_MAX_BINS 4096" in hdr and _lib.SWEEP_MAX_BINS == 4096
    assert "#define USSEG_TEMP_MAX_BETAS 16" in hdr and _lib.TEMP_MAX_BETAS == 16
    assert "#define USSEG_TEMP_NLL_CAP 1024" in hdr and _lib.TEMP_NLL_CAP == 1024 and _lib.TEMP_NLL_UNIT == 2.0 ** -20
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    assert sum("operating_point.hip" in line for line in mk.splitlines() if line.startswith(("SRCS", "NOPK_SRCS"))) == 2


# ------------------------------------------------------------------------------------------------ argument checks (no launch: no device needed)
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _sweep(B=1, H=4, W=4, C_=3, bins=64, cls=2, probs=16, y=32, counts=48):
    L, lib = _lib()
    return lib.usseg_score_sweep(C.byref(L.SweepDesc(B, H, W, C_, bins, cls)), probs, y, counts, None), lib.usseg_last_error()


def test_score_sweep_rejects_bad_arguments():
    L, lib = _lib()
    assert lib.usseg_score_sweep(None, 16, 32, 48, None) == -1
    for kw in (dict(probs=None), dict(y=None), dict(counts=None)):
        rc, msg = _sweep(**kw)
        assert rc == -1 and b"score_sweep: null pointer" in msg, kw
    for b in (0, 1, 3, 48, 1000, 4097, 8192, -4):
        rc, msg = _sweep(bins=b)
        assert rc == -1 and b"bins is a power of two, 2 <= bins <= 4096" in msg, b
    for c in (0, 5):
        rc, msg = _sweep(C_=c, cls=0)
        assert rc == -1 and b"1 <= C <= 4" in msg, c
    for cls, c in ((3, 3), (2, 2), (4, 4), (-1, 3)):
        rc, msg = _sweep(cls=cls, C_=c)
        assert rc == -1 and b"cls is a class below C" in msg, (cls, c)
    for kw in (dict(B=-1), dict(H=-1), dict(W=0)):
        rc, msg = _sweep(**kw)
        assert rc == -1 and b"score_sweep: bad descriptor (B, H" in msg, kw
    rc, msg = _sweep(B=1 << 15, H=1 << 15, W=4)
    assert rc == -1 and b"B*H*W <= 2^31" in msg
    assert _sweep(B=0)[0] == 0 and _sweep(H=0)[0] == 0          # an empty batch: nothing to count, nothing launched


def _nll(betas=(1.0,), n=None, B=1, H=4, W=4, C_=3, probs=16, y=32, counts=48, null_betas=False):
    L, lib = _lib()
    arr = None if null_betas else (C.c_float * max(len(betas), 1))(*betas)
    d = L.TempDesc(B, H, W, C_, len(betas) if n is None else n)
    return lib.usseg_temperature_nll(C.byref(d), probs, y, arr, counts, None), lib.usseg_last_error()


def test_temperature_nll_rejects_bad_arguments():
    L, lib = _lib()
    assert lib.usseg_temperature_nll(None, 16, 32, (C.c_float * 1)(1.0), 48, None) == -1
    for kw in (dict(probs=None), dict(y=None), dict(counts=None), dict(null_betas=True)):
        rc, msg = _nll(**kw)
        assert rc == -1 and b"temperature_nll: null pointer" in msg, kw
    for n in (0, 17, -1):
        rc, msg = _nll(betas=(1.0,) * 17, n=n)
        assert rc == -1 and b"1 <= n_beta <= 16" in msg, n
    for bad in (0.0, -1.0, 16.5, float("inf"), float("nan")):
        rc, msg = _nll(betas=(1.0, bad))
        assert rc == -1 and b"beta 1 must be finite with 0 < beta <= 16" in msg, bad
    for c in (0, 5):
        rc, msg = _nll(C_=c)
        assert rc == -1 and b"temperature_nll: bad descriptor (1 <= C <= 4)" in msg
    rc, msg = _nll(W=0)
    assert rc == -1 and b"temperature_nll: bad descriptor (B, H" in msg
    assert _nll(B=0)[0] == 0 and _nll(betas=(0.125, 16.0), H=0)[0] == 0


def test_apply_temperature_rejects_bad_arguments():
    L, lib = _lib()
    d = L.TempDesc(1, 4, 4, 3, 1)
    assert lib.usseg_apply_temperature(None, 16, 32, 48, None) == -1
    for args in ((None, 32, 48), (16, None, 48), (16, 32, None)):
        assert lib.usseg_apply_temperature(C.byref(d), *args, None) == -1 and b"apply_temperature: null pointer" in lib.usseg_last_error()
    for d in (L.TempDesc(1, 4, 4, 0, 1), L.TempDesc(1, 4, 4, 5, 1), L.TempDesc(-1, 4, 4, 3, 1), L.TempDesc(1, 4, 0, 3, 1), L.TempDesc(1 << 16, 1 << 16, 1, 3, 1)):
        assert lib.usseg_apply_temperature(C.byref(d), 16, 32, 48, None) == -1 and b"apply_temperature: bad descriptor" in lib.usseg_last_error()
    assert lib.usseg_apply_temperature(C.byref(L.TempDesc(0, 4, 4, 3, 0)), 16, 32, 48, None) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_wrappers_refuse_bad_arguments():
    import torch
    from ultrasound_modeling_amd import metrics, ops
    p = torch.zeros(1, 2, 2, 3)
    for bins in (0, 3, 1000, 8192):
        with pytest.raises(ValueError, match="power of two"):
            ops.score_sweep(p, p, torch.zeros(2 * max(bins, 1) + 1, dtype=torch.int64), bins=bins)
        with pytest.raises(ValueError, match="power of two"):
            metrics.SweepCounts(bins, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_sweep(p, p, torch.zeros(129, dtype=torch.int64), bins=64)
    with pytest.raises(ValueError, match="betas"):
        ops.temperature_nll(p, p, [1.0] * 17, torch.zeros(19, dtype=torch.int64))
    with pytest.raises(ValueError, match="betas"):
        ops.temperature_nll(p, p, [], torch.zeros(2, dtype=torch.int64))
    for bad in (0.0, -2.0, 17.0, float("nan")):
        with pytest.raises(ValueError, match="0 < beta <= 16"):
            ops.temperature_nll(p, p, [1.0, bad], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.temperature_nll(p, p, [1.0], torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.apply_temperature(p, torch.ones(1))
    with pytest.raises(ValueError, match="cls"):
        metrics.SweepCounts(64, cls=4, device="cpu")
    sw = metrics.SweepCounts(64, device="cpu")           # the counters alone need no device
    assert sw.counts.shape == (129,) and math.isnan(sw.result()["auc"])


def test_cascade_temperature_refusals_and_the_drivers_option_checks():
    from ultrasound_modeling_amd import TBIEvaluator as T
    from ultrasound_modeling_amd.MainNumpy import Process
    for bad in (0.0, -1.0, 1 / 32, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            T._beta_of(bad)
    assert T._beta_of(2.0) == 0.5 and T._beta_of(1 / 16) == 16.0
    base = ["d.npy", "p.npy", "axes", "out", "--bleed", "b.ckpt"]
    for extra in (["--sweep-bins", "1000"], ["--sweep-bins", "8192"], ["--temperature", "0"], ["--temperature", "2", "--fit-temperature"],
                  ["--threshold", "best"], ["--threshold", "nan"]):
        with pytest.raises(SystemExit):
            T.main(base + extra)
    with pytest.raises(ValueError, match="sweep takes a dict"):
        Process(batch_size=2, num_classes=3, device="cpu", sweep={"bin": 64})
    assert T.SWEEP_COLUMNS == ("k", "threshold", "tp", "fp", "fn", "tn", "tpr", "fpr", "precision", "dice")


def test_write_roc_csv(tmp_path):
    import csv
    from ultrasound_modeling_amd import TBIEvaluator as T
    from ultrasound_modeling_amd.metrics import sweep_from_counts
    p = tmp_path / "roc.csv"
    assert T.write_roc_csv(p, sweep_from_counts(np.array([3, 1, 1, 3, 2]))) == 3
    rows = list(csv.reader(open(p)))
    assert len(rows) == 5 and rows[0][:10] == list(T.SWEEP_COLUMNS)
    assert rows[1][:10] == ["0", "-inf", "4", "4", "0", "0", "1.0", "1.0", "0.5", repr(8 / 12)]
    assert rows[2][:6] == ["1", repr(float(np.nextafter(np.float32(0.5), np.float32(0)))), "3", "1", "1", "3"]
    assert rows[4][0] == "total" and rows[4][10:] == ["8", "0.75", repr(0.25 * 0.5 + 0.75 * 0.75), "1", rows[2][1], "0.75", "1", rows[2][1], "0.5", "2"]
