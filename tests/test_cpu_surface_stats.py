"""HD95 and the surface Dice without a GPU: the restatement (tests/surface_restatement.py) against SciPy and NumPy and against known answers,
the host arithmetic (``metrics.surface_scores_from_stats``, ``metrics.tolerance_squared``) against the restatement, the C ABI of
``usseg_surface_stats`` (symbols, workspace formula, every argument check before any launch), the evaluator's CSV header and command line.

The bound of the NumPy comparison.  ``np.percentile`` computes its virtual index by another formula than ``q / 100 * (n - 1)``, so that
comparison is not bitwise:  |diff| <= 8 * eps * max(pos, 1) * (hi - lo) + 4 * ulp(value)  - the index differs by a few ulp of pos, which moves
the lerp by that times the gap between the two neighbouring distances; the lerp itself has three roundings.  The worst observed ratio to the bound is printed.
"""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import boundary_restatement as BR
import surface_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0, 5, 50, 95, 99.9, 100)
EPS = 2.0 ** -52


def _masks(H, W, da, db, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.random((H, W)) < da, rng.random((H, W)) < db
    a[0, 0] = b[H - 1, W - 1] = True
    return a, b


# ------------------------------------------------------------------------------------------------ the restatement against SciPy and NumPy
@pytest.mark.parametrize("H,W,da,db", [(5, 7, 0.3, 0.3), (33, 19, 0.3, 0.02), (37, 130, 0.3, 0.02), (1, 9, 0.5, 0.2)])
def test_the_integer_multisets_equal_scipys_transform(H, W, da, db):
    nd = pytest.importorskip("scipy.ndimage")
    a, b = _masks(H, W, da, db, 100 * H + W)
    c, d = SR.sets(a, b)
    sa, sb = BR.surface(a), BR.surface(b)
    want_ab = np.sort(np.rint(nd.distance_transform_edt(~sb)[sa] ** 2).astype(np.int64))
    want_ba = np.sort(np.rint(nd.distance_transform_edt(~sa)[sb] ** 2).astype(np.int64))
    assert np.array_equal(d[0], want_ab) and np.array_equal(d[1], want_ba) and np.array_equal(d[2], np.sort(np.concatenate([want_ab, want_ba])))
    assert c == [len(want_ab), len(want_ba), int(want_ab.max()), int(want_ba.max())]


def test_the_issues_figures_at_37_by_130():
    """``rand < 0.3`` against ``rand < 0.02``, seed fixed: the surface sizes and the pooled HD95 to four decimals."""
    rng = np.random.default_rng(0)
    a, b = rng.random((37, 130)) < 0.3, rng.random((37, 130)) < 0.02
    c, d = SR.sets(a, b)
    assert c == [1432, 80, 157, 5] and len(d[2]) == 1512
    assert round(SR.percentile(95, d[2]), 4) == 7.2111 and SR.percentile(95, d[2]) == math.sqrt(52) and SR.percentile(100, d[2]) == math.sqrt(157)
    w = np.zeros((1, 4200), bool), np.zeros((1, 4200), bool)         # a at x = 0 and 10, b at x = 4199: squares of 2^24 and more
    w[0][0, 0] = w[0][0, 10] = w[1][0, 4199] = True
    c, d = SR.sets(*w)
    assert d[2].tolist() == [17547721, 17547721, 17631601] and d[2][0] >= 2 ** 24 and SR.percentile(95, d[2]) == 4198.0


def test_percentiles_against_numpy_within_the_stated_bound():
    worst = 0.0
    for H, W, da, db, seed in ((5, 7, 0.3, 0.3, 1), (33, 19, 0.3, 0.02, 2), (37, 130, 0.3, 0.02, 3), (37, 130, 0.5, 0.5, 4), (1, 40, 0.2, 0.1, 5)):
        a, b = _masks(H, W, da, db, seed)
        c, d = SR.sets(a, b)
        roots = [np.sqrt(s.astype(np.float64)) for s in d]
        for q in QS:
            for which in ("pooled", "directed"):
                if which == "pooled":
                    got, want, sets_ = SR.percentile(q, d[2]), float(np.percentile(np.hstack((roots[0], roots[1])), q)), [2]
                else:
                    got = max(SR.percentile(q, d[0]), SR.percentile(q, d[1]))
                    want, sets_ = max(float(np.percentile(roots[0], q)), float(np.percentile(roots[1], q))), [0, 1]
                bound = 0.0
                for s in sets_:                                     # (directed: the larger of the two sets' bounds covers the larger of the values)
                    pos, k, k1 = SR.ranks(q, len(d[s]))
                    lo, hi = math.sqrt(int(d[s][k])), math.sqrt(int(d[s][k1]))
                    value = SR.percentile(q, d[s])
                    bound = max(bound, 8 * EPS * max(pos, 1) * (hi - lo) + 4 * math.ulp(value))
                diff = abs(got - want)
                assert diff <= bound, (H, W, q, which, got, want, diff, bound)
                worst = max(worst, diff / bound if bound else 0.0)
    print(f"\n  worst |restatement - np.percentile| / bound = {worst:.3f}", end="")


# ------------------------------------------------------------------------------------------------ known answers
def test_identical_masks():
    a, _ = _masks(9, 11, 0.4, 0.4, 7)
    r = SR.scores(a, a, QS, (0, 1))
    assert r["pooled"] == [0.0] * 6 and r["directed"] == [0.0] * 6 and r["nsd"] == [1.0, 1.0]
    assert all(p == (0, 0) for s in r["sel"] for p in s)


def test_one_pixel_against_one_pixel():
    a, b = np.zeros((5, 7), bool), np.zeros((5, 7), bool)
    a[1, 1] = b[4, 5] = True
    r = SR.scores(a, b, QS, (4, 5))
    assert r["counters"] == [1, 1, 25, 25]
    for q in QS:
        assert SR.ranks(q, 1) == (0.0, 0, 0)                        # n = 1 per direction: k = k1 = 0 whatever q
    assert r["sel"][0] == [(25, 25)] * 6 and r["sel"][1] == [(25, 25)] * 6 and r["directed"] == [5.0] * 6 and r["pooled"] == [5.0] * 6
    assert r["nsd"] == [0.0, 1.0] and r["within"] == [(0, 0), (1, 1)]


def test_a_set_of_two():
    a, b = np.zeros((1, 12), bool), np.zeros((1, 12), bool)
    a[0, 0] = a[0, 4] = True                                        # distances to b at x = 10: 10 and 6
    b[0, 10] = True
    c, d = SR.sets(a, b)
    assert d[0].tolist() == [36, 100] and d[1].tolist() == [36] and d[2].tolist() == [36, 36, 100]
    assert SR.ranks(50, 2) == (0.5, 0, 1) and SR.percentile(50, d[0]) == 8.0 and SR.percentile(0, d[0]) == 6.0 and SR.percentile(100, d[0]) == 10.0
    assert SR.pair(95, d[0]) == (36, 100) and SR.percentile(95, d[0]) == 6.0 + 4.0 * (95 / 100 * 1)
    assert SR.percentile(95, d[2]) == 6.0 + 4.0 * (95 / 100 * 2 - 1)


def test_tolerances_around_the_square_root_of_two():
    from ultrasound_modeling_amd.metrics import tolerance_squared
    r2 = math.sqrt(2.0)
    below, above = math.nextafter(r2, 0.0), math.nextafter(r2, 2.0)
    for tau, want in ((1, 1), (below, 1), (r2, 2), (above, 2), (0, 0), (0.999, 0), (2, 4), (1e3, 10 ** 6), (3.5, 12), (math.sqrt(3.0), 3),
                      (math.nextafter(math.sqrt(3.0), 0.0), 2), (math.sqrt(17631601.0 + 1), 17631602)):
        assert tolerance_squared(tau) == SR.tol2(tau) == want, tau
        assert math.isqrt(want) <= tau and math.sqrt(want) <= tau < math.sqrt(want + 1)
    from fractions import Fraction
    assert Fraction(math.sqrt(3.0)) ** 2 < 3 < Fraction(r2) ** 2 + 1         # math.sqrt(3) lies BELOW the real root and still admits the pixel at math.sqrt(3):
    #                                                                          floor(tau^2) alone would say 2
    for bad in (-1.0, float("nan"), float("inf"), 50000.0):
        with pytest.raises(ValueError):
            tolerance_squared(bad)


def test_zero_tolerance_counts_the_shared_surface_pixels():
    a, b = np.zeros((6, 8), bool), np.zeros((6, 8), bool)
    a[2, 1:5] = True
    b[2, 3:7] = True
    r = SR.scores(a, b, (), (0,))
    assert r["within"] == [(2, 2)] and r["nsd"] == [4 / 8]


def test_empty_surfaces():
    e, m = np.zeros((4, 6), bool), np.ones((4, 6), bool)
    r = SR.scores(e, m, (95,), (2,))
    assert r["sel"] == [[(-1, -1)]] * 3 and math.isnan(r["pooled"][0]) and math.isnan(r["directed"][0]) and r["nsd"] == [0.0]
    r = SR.scores(e, e, (95,), (2,))
    assert math.isnan(r["pooled"][0]) and math.isnan(r["nsd"][0])


def test_the_host_arithmetic_equals_the_restatement_bit_for_bit():
    """``metrics.surface_scores_from_stats`` fed with the integers the device would return."""
    import torch
    from ultrasound_modeling_amd.metrics import surface_scores_from_stats
    pairs = [_masks(33, 19, 0.3, 0.05, 1), _masks(33, 19, 0.5, 0.5, 2), (np.zeros((33, 19), bool), _masks(33, 19, 0.3, 0.3, 3)[1]),
             (np.zeros((33, 19), bool),) * 2]
    taus = (0, 1.5, 3)
    rows = [SR.scores(a, b, QS[:4], taus) for a, b in pairs]
    counters = torch.tensor([r["counters"] for r in rows])
    sums = torch.zeros((4, 2), dtype=torch.float64)
    sel = torch.tensor([[[list(p) for p in s] for s in r["sel"]] for r in rows], dtype=torch.int32)
    within = torch.tensor([[list(w) for w in r["within"]] for r in rows])
    s = surface_scores_from_stats(counters, sums, sel, within, QS[:4], taus)
    same = lambda x, y: (math.isnan(x) and math.isnan(y)) or float(x).hex() == float(y).hex()
    for i, r in enumerate(rows):
        assert all(same(s["hd_pct"][i, p], r["pooled"][p]) and same(s["hd_pct_directed"][i, p], r["directed"][p]) for p in range(4)), i
        assert all(same(s["nsd"][i, t], r["nsd"][t]) for t in range(3)), i
    assert s["percentiles"] == [0.0, 5.0, 50.0, 95.0] and s["tolerances"] == [0.0, 1.5, 3.0]
    for bad in ((101,), (-1,), (float("nan"),), (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError):
            surface_scores_from_stats(counters, sums, sel, within, bad, ())


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def test_exported_symbols_and_header_text():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in ("usseg_surface_stats_ws_bytes", "usseg_surface_stats"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in hdr, name
    for text in ("pos = t * (double)(n - 1)", "k1 = min(k + 1, n - 1)", "value = lo + (hi - lo) * g", "np.percentile(np.hstack((d_ab, d_ba)), 95)",
                 "sel    int32 [N,3,P,2]", "within int64 [N,T,2]", "round16(4*N*H*W) + round16(8*N*H*W)"):
        assert text in hdr, text
    assert "is not provided" not in hdr


def test_workspace_sizes():
    L, lib = _lib()
    r16 = lambda v: (v + 15) // 16 * 16
    for N, H, W in ((16, 256, 80), (3, 5, 7), (1, 1, 1), (0, 4, 4)):
        assert lib.usseg_surface_stats_ws_bytes(N, H, W) == r16(4 * N * H * W) + r16(8 * N * H * W), (N, H, W)
    assert lib.usseg_surface_stats_ws_bytes(16, 256, 80) == 12 * 16 * 256 * 80 and lib.usseg_surface_stats_ws_bytes(3, 5, 7) == 432 + 848
    for bad in ((1, 0, 8), (1, 8, 0), (1, 8193, 8), (1, 8, 8193), (-1, 8, 8)):
        assert lib.usseg_surface_stats_ws_bytes(*bad) == -1, bad
    from ultrasound_modeling_amd import ops
    with pytest.raises(ValueError):
        ops.surface_stats_ws_bytes(1, 0, 8)


def test_surface_stats_refuses_bad_arguments_before_any_launch():
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(a=16, b=16, N=1, H=8, W=8, quant=(0.95,), tol2=(2,), counters=16, sums=16, sel=16, within=16, ws=16, ws_bytes=1 << 20, P=None, T=None):
        qa = None if quant is None else (C.c_double * max(len(quant), 1))(*quant)
        ta = None if tol2 is None else (C.c_int32 * max(len(tol2), 1))(*tol2)
        P = (len(quant) if quant is not None else 0) if P is None else P
        T = (len(tol2) if tol2 is not None else 0) if T is None else T
        return lib.usseg_surface_stats(a, b, N, H, W, qa, P, ta, T, counters, sums, sel, within, ws, ws_bytes, None)

    for kw in (dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(H=-3)):
        assert call(**kw) == -1 and "surface_stats: H and W must lie in [1, 8192]" in err(), kw
    for n in (-1, 65536):
        assert call(N=n) == -1 and "surface_stats: 0 <= N <= 65535" in err()
    assert call(N=9, H=8192, W=8192, ws_bytes=1 << 40) == -1 and "more than 2^29 pixels" in err()
    for p in (-1, 5):
        assert call(P=p) == -1 and "quantiles" in err()
    for t in (-1, 5):
        assert call(T=t) == -1 and "tolerances" in err()
    for kw in (dict(a=None), dict(b=None), dict(counters=None), dict(sums=None), dict(ws=None), dict(sel=None), dict(within=None), dict(quant=None, P=1),
               dict(tol2=None, T=1)):
        assert call(**kw) == -1 and "surface_stats: null pointer" in err(), kw
    for q in (1.0000001, -1e-9, float("nan"), float("inf")):
        assert call(quant=(0.5, q)) == -1 and "must be finite and lie in [0, 1]" in err(), q
    assert call(tol2=(3, -1)) == -1 and "squared tolerance 1 must be >= 0" in err()
    for kw in (dict(counters=20), dict(sums=12), dict(within=12), dict(sel=18), dict(ws=8)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    need = lib.usseg_surface_stats_ws_bytes(1, 8, 8)
    assert need == 768 and call(ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    assert call(N=0) == 0                                                          # nothing to do, nothing launched
    assert call(N=0, quant=(), tol2=(), sel=None, within=None) == 0               # P == 0, T == 0: their outputs may be null
    assert call(N=0, quant=None, tol2=None, sel=None, within=None) == 0


def test_ops_refuses_what_the_library_would():
    import torch
    from ultrasound_modeling_amd import ops
    m = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for kw in (dict(percentiles=(1, 2, 3, 4, 5)), dict(tol2=(1,) * 5), dict(percentiles=(100.00001,)), dict(percentiles=(float("nan"),)), dict(tol2=(-1,)),
               dict(tol2=(1.5,))):
        with pytest.raises(ValueError):
            ops.surface_stats(m, m, **kw)
    par = inspect.signature(ops.surface_stats).parameters
    assert list(par) == ["a", "b", "percentiles", "tol2", "ws", "out"] and par["ws"].kind is par["out"].kind is inspect.Parameter.KEYWORD_ONLY


# ------------------------------------------------------------------------------------------------ the evaluator and the drivers
def test_the_csv_without_the_new_arguments_is_todays(tmp_path, monkeypatch):
    from ultrasound_modeling_amd import TBIEvaluator as E
    calls, real = [], E.surface_scores

    def stub(result, threshold=0.5, device=None, *, pred_mask=None):               # today's signature: the new keywords are not passed on
        calls.append(1)
        return {"hd": np.array([2.0, np.nan]), "assd": np.array([0.5, np.nan]), "n_a": np.array([3, 0]), "n_b": np.array([4, 5])}

    monkeypatch.setattr(E, "surface_scores", stub)
    z = np.zeros((2, 4, 4), np.float32)
    res = E.PolarResult(z, z, None, z, z, np.asarray(["p", "q"]))
    assert E.write_surface_csv(tmp_path / "s.csv", res) == 2 and calls == [1]
    assert open(tmp_path / "s.csv", newline="").read() == "name,hd,assd,n_pred,n_label\r\np,2.0,0.5,3,4\r\nq,nan,nan,0,5\r\n"
    for fn in (real, E.write_surface_csv):
        par = inspect.signature(fn).parameters
        assert par["percentiles"].default is None and par["tolerances"].default is None and par["percentiles"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_command_line_and_the_drivers_signatures(capsys):
    from ultrasound_modeling_amd import MainNumpy, TBIEvaluator, metrics
    src = inspect.getsource(TBIEvaluator.main)
    assert "--surface-percentile" in src and "--surface-tolerance" in src
    for extra in (["--surface-percentile", "95"], ["--surface-tolerance", "2"]):
        with pytest.raises(SystemExit):
            TBIEvaluator.main(["d.npy", "p.npy", "axes", "out", "--bleed", "b.ckpt"] + extra)
        assert "need --surface-csv" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        TBIEvaluator.main(["d.npy", "p.npy", "axes", "out", "--bleed", "b.ckpt", "--surface-csv", "s.csv"] + ["--surface-percentile", "95"] * 5)
    assert "at most 4" in capsys.readouterr().err
    par = inspect.signature(MainNumpy.Process.__init__).parameters
    assert par["surface"].default is None
    assert MainNumpy.surface_settings(dict(percentiles=[95], tolerances=[2])) == {"percentiles": [95.0], "tolerances": [2.0], "tol2": [4]}
    for bad in (dict(percentile=[95]), [95], dict(percentiles=[101]), dict(tolerances=[-1])):
        with pytest.raises(ValueError):
            MainNumpy.surface_settings(bad)
    par = inspect.signature(metrics.surface_distances).parameters
    assert par["percentiles"].default is None and par["tolerances"].default is None and par["tolerances"].kind is inspect.Parameter.KEYWORD_ONLY
