"""HD95 / surface Dice on the GPU (usseg.h: usseg_surface_stats; csrc/sdf.hip) against the restatement (tests/surface_restatement.py).

Every comparison is exact: integers (counters, the selected squared distances, the counts within a tolerance) are equal, fp64 values (the
sums, the percentiles, the surface Dice) have equal BITS - the host arithmetic is the restatement's, operation for operation.  Nothing is left out
of any check.  ``counters`` and ``sums`` are compared with ``ops.surface_dist``'s on the same masks, bit for bit, in every case.
"""
import csv
import functools
import io
import contextlib
import math
import random
import struct

import numpy as np
import pytest
import torch

import surface_restatement as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q4, Q1 = (0, 50, 99.9, 100), (95,)
T4, T1 = (0, 1, 2, 10 ** 6), (2,)


def _bits(x):
    return struct.pack("<d", float(x))


def _pair(kind, H, W, rng):
    a, b = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    if kind == "rand":
        a[:] = rng.random((H, W)) < 0.3
        b[:] = rng.random((H, W)) < 0.02
        a[0, 0] = 1
        b[H - 1, W - 1] = 1
    elif kind == "seed0":                                 # 1432 and 80 surface pixels, maxima 157 and 5, pooled HD95 7.2111 (tests/test_cpu_surface_stats.py)
        rng = np.random.default_rng(0)
        a[:] = rng.random((H, W)) < 0.3
        b[:] = rng.random((H, W)) < 0.02
    elif kind == "mixed":
        a[:] = rng.random((H, W)) < 0.5
        b[:] = rng.random((H, W)) < 0.5
        a[0, 0] = b[H - 1, 0] = 1
    elif kind == "far_blobs":
        a[2:9, 3:11] = 1
        b[H - 8:H - 2, W - 20:W - 5] = 3                  # any nonzero byte is inside
    elif kind == "full":
        a[:], b[:] = 1, 1
        b[:, W // 2:] = 0
    elif kind == "identical":
        a[:] = rng.random((H, W)) < 0.4
        a[H // 2, W // 2] = 1
        b[:] = a
    elif kind == "all_equal":                             # every pixel of either surface is 5 from the other: two parallel lines
        a[4, :] = 1
        b[9, :] = 1
    elif kind == "a_empty":
        b[:] = rng.random((H, W)) < 0.2
        b[1, 1] = 1
    elif kind == "b_empty":
        a[:] = rng.random((H, W)) < 0.6
        a[1, 1] = 1
    elif kind == "both_empty":
        pass
    elif kind == "wide":                                  # squares of 2^24 and more: the top digit of the select
        a[0, 0] = a[0, 10] = 1
        b[0, W - 1] = 1
    else:
        raise KeyError(kind)
    return a, b


@functools.lru_cache(maxsize=None)
def _case(kinds, H, W):
    """-> a, b uint8 [N,H,W] and, per image, the restatement's (counters, [sorted D_ab, D_ba, D_pool]) - computed once."""
    rng = np.random.default_rng(1000 * H + W)
    pairs = [_pair(k, H, W, rng) for k in kinds]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return a, b, [SR.sets(p[0], p[1]) for p in pairs]


def _call(ad, bd, qs, t2s):
    """One call into sentinel-filled outputs -> four CPU arrays."""
    from ultrasound_modeling_amd import ops
    N = ad.shape[0]
    out = (torch.full((N, 4), -77, dtype=torch.int64, device=DEV), torch.full((N, 2), float("nan"), dtype=torch.float64, device=DEV),
           torch.full((N, 3, len(qs), 2), -77, dtype=torch.int32, device=DEV), torch.full((N, len(t2s), 2), -77, dtype=torch.int64, device=DEV))
    got = ops.surface_stats(ad, bd, qs, t2s, out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    return [g.cpu().numpy() for g in got]


def _check(kinds, H, W, qs, t2s):
    from ultrasound_modeling_amd import ops
    a, b, ref = _case(kinds, H, W)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    counters, sums, sel, within = _call(ad, bd, qs, t2s)
    c0, s0 = ops.surface_dist(ad, bd)
    torch.cuda.synchronize()
    assert np.array_equal(counters, c0.cpu().numpy()), (kinds, counters, c0)
    assert np.array_equal(sums.view(np.int64), s0.cpu().numpy().view(np.int64)), (kinds, sums, s0)                # bit for bit
    for i, (cnt, d) in enumerate(ref):
        assert counters[i].tolist() == cnt, (kinds[i], counters[i], cnt)
        for s in range(3):
            for p, q in enumerate(qs):
                assert tuple(sel[i, s, p].tolist()) == SR.pair(q, d[s]), (kinds[i], s, q, sel[i, s, p], SR.pair(q, d[s]), len(d[s]))
                if q == 100 and s < 2:
                    assert sel[i, s, p, 0] == sel[i, s, p, 1] == counters[i, 2 + s]                              # the maxima
        for t, t2 in enumerate(t2s):
            assert within[i, t].tolist() == [int((d[0] <= t2).sum()), int((d[1] <= t2).sum())], (kinds[i], t2, within[i, t])
    for _ in range(2):                                                                                          # three calls, the same bits
        again = _call(ad, bd, qs, t2s)
        for g, w in zip(again, (counters, sums, sel, within)):
            assert g.tobytes() == w.tobytes()
    return counters, sums, sel, within


@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (2, 64), (3, 65), (37, 130), (16, 256)])
def test_every_shape_equals_the_restatement(H, W):
    for qs, t2s in ((Q4, T4), (Q1, T1)):
        _check(("mixed", "rand"), H, W, qs, t2s)


def test_squares_of_two_to_the_24_and_more():
    counters, sums, sel, within = _check(("wide",), 1, 4200, Q1 + (0, 100), T1)
    assert counters[0].tolist() == [2, 1, 4199 ** 2, 4189 ** 2] and 4189 ** 2 >= 2 ** 24
    # D_ab = {4189^2, 4199^2}: q = 0 has k = 0 and k1 = min(1, n - 1) = 1; q = 100 has k = k1 = 1.  D_ba = {4189^2}: n = 1
    assert sel[0, 0, 1].tolist() == [4189 ** 2, 4199 ** 2] and sel[0, 0, 2].tolist() == [4199 ** 2] * 2 and sel[0, 1, 0].tolist() == [4189 ** 2] * 2
    assert sel[0, 2, 0].tolist() == [4189 ** 2, 4199 ** 2]      # pooled {4189^2, 4189^2, 4199^2} at q = 95: pos = 1.9, ranks 1 and 2
    from ultrasound_modeling_amd.metrics import surface_scores_from_stats
    assert surface_scores_from_stats(counters, sums, sel, within, Q1 + (0, 100), (math.sqrt(2),))["hd_pct"][0, 0] == 4198.0


@pytest.mark.parametrize("kinds", [("seed0",), ("far_blobs",), ("full",), ("identical",), ("all_equal",)])
def test_contents_at_37_by_130(kinds):
    for qs, t2s in ((Q4, T4), (Q1, T1)):
        counters, sums, sel, within = _check(kinds, 37, 130, qs, t2s)
    if kinds == ("seed0",):
        assert counters[0].tolist() == [1432, 80, 157, 5] and sel[0, 2, 0].tolist() == [52, 52]                 # sqrt(52) = 7.2111
    if kinds == ("identical",):
        assert not sel.any() and within[0, 0].tolist() == counters[0, :2].tolist()
    if kinds == ("all_equal",):
        assert (sel == 25).all() and counters[0].tolist() == [130, 130, 25, 25]
    if kinds == ("full",):
        assert counters[0, 0] == 2 * 37 + 2 * 130 - 4                                                           # the image border


@pytest.mark.parametrize("P,T", [(0, 0), (1, 0), (0, 1), (4, 0), (0, 4), (4, 4), (1, 4)])
def test_every_count_of_percentiles_and_tolerances(P, T):
    counters, sums, sel, within = _check(("rand", "mixed"), 37, 130, {0: (), 1: Q1, 4: Q4}[P], {0: (), 1: T1, 4: T4}[T])
    assert sel.shape == (2, 3, P, 2) and within.shape == (2, T, 2)


def test_empty_surfaces_and_a_permutation_of_the_rows():
    kinds = ("a_empty", "b_empty", "rand")
    first = _check(kinds, 37, 130, Q4, T4)
    assert first[0][0, 2:].tolist() == [-1, -1] and (first[2][:2] == -1).all() and not first[3][:2].any() and first[0][1, 0] > 0
    a, b, _ = _case(kinds, 37, 130)
    perm = [2, 0, 1]
    got = _call(torch.from_numpy(a[perm].copy()).to(DEV), torch.from_numpy(b[perm].copy()).to(DEV), Q4, T4)
    for g, w in zip(got, first):
        assert g.tobytes() == w[perm].tobytes()                                                                 # the rows permute, nothing else changes
    both = _check(("both_empty",), 37, 130, Q4, T4)
    assert both[0].tolist() == [[0, 0, -1, -1]] and (both[2] == -1).all() and not both[3].any() and not both[1].any()


def test_no_images():
    from ultrasound_modeling_amd import ops
    e = torch.zeros((0, 5, 7), dtype=torch.uint8, device=DEV)
    counters, sums, sel, within = ops.surface_stats(e, e, Q1, T1)
    assert counters.shape == (0, 4) and sums.shape == (0, 2) and sel.shape == (0, 3, 1, 2) and within.shape == (0, 1, 2)


def test_a_captured_call_follows_the_masks():
    from ultrasound_modeling_amd import ops
    a, b, _ = _case(("rand", "mixed", "far_blobs"), 37, 130)
    a2, b2, _ = _case(("mixed", "identical", "b_empty"), 37, 130)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ws = torch.zeros(ops.surface_stats_ws_bytes(3, 37, 130), dtype=torch.uint8, device=DEV)
    out = (torch.zeros((3, 4), dtype=torch.int64, device=DEV), torch.zeros((3, 2), dtype=torch.float64, device=DEV),
           torch.zeros((3, 3, 4, 2), dtype=torch.int32, device=DEV), torch.zeros((3, 4, 2), dtype=torch.int64, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.surface_stats(ad, bd, Q4, T4, ws=ws, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.surface_stats(ad, bd, Q4, T4, ws=ws, out=out)                 # one linear chain of three launches
    ad.copy_(torch.from_numpy(a2))
    bd.copy_(torch.from_numpy(b2))
    want = _call(ad.clone(), bd.clone(), Q4, T4)
    for _ in range(2):
        for o in out:
            o.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, want):
            assert o.cpu().numpy().tobytes() == w.tobytes()


def test_refusals_leave_the_outputs_alone():
    import ctypes as C
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    a, b, _ = _case(("rand",), 37, 130)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    need = ops.surface_stats_ws_bytes(1, 37, 130)
    big = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)

    def fresh():
        return (torch.full((1, 4), -77, dtype=torch.int64, device=DEV), torch.full((1, 2), -77.0, dtype=torch.float64, device=DEV),
                torch.full((1, 3, 1, 2), -77, dtype=torch.int32, device=DEV), torch.full((1, 1, 2), -77, dtype=torch.int64, device=DEV))

    for ws, text in ((big[:need - 1], f"the workspace holds {need - 1} bytes, {need} needed"), (big[8:8 + need], "aligned")):
        out = fresh()
        with pytest.raises(L.UssegError, match=text):
            ops.surface_stats(ad, bd, Q1, T1, ws=ws, out=out)
        torch.cuda.synchronize()
        assert all(bool((o == -77).all()) for o in out)
    out = fresh()
    rc = L.load().usseg_surface_stats(ad.data_ptr(), bd.data_ptr(), 1, 37, 130, (C.c_double * 1)(1.0000001), 1, (C.c_int32 * 1)(2), 1, out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), big.data_ptr(), big.numel(), None)
    torch.cuda.synchronize()
    assert rc == -1 and "must be finite and lie in [0, 1]" in L.load().usseg_last_error().decode()
    assert all(bool((o == -77).all()) for o in out)


# ------------------------------------------------------------------------------------------------ the Python layers
def test_metrics_surface_distances_equals_the_restatement_bit_for_bit():
    from ultrasound_modeling_amd.metrics import surface_distances
    kinds = ("rand", "mixed", "a_empty", "b_empty", "both_empty", "identical", "far_blobs")
    a, b, _ = _case(kinds, 37, 130)
    taus = (1, 2)
    s = surface_distances(a, b.astype(bool), percentiles=(95,), tolerances=taus)
    plain = surface_distances(a, b)
    assert set(plain) == {"hd", "assd", "n_a", "n_b", "max_ab", "max_ba", "sum_ab", "sum_ba"}                   # without the keywords: today's keys
    assert set(s) == set(plain) | {"hd_pct", "hd_pct_directed", "nsd", "percentiles", "tolerances", "sel", "within"}
    for k in plain:
        assert s[k].tobytes() == plain[k].tobytes(), k
    assert s["percentiles"] == [95.0] and s["tolerances"] == [1.0, 2.0] and s["hd_pct"].shape == (7, 1) and s["nsd"].shape == (7, 2)
    for i, kind in enumerate(kinds):
        r = SR.scores(a[i], b[i], (95,), taus)
        assert _bits(s["hd_pct"][i, 0]) == _bits(r["pooled"][0]) and _bits(s["hd_pct_directed"][i, 0]) == _bits(r["directed"][0]), (kind, s["hd_pct"][i], r)
        assert [_bits(v) for v in s["nsd"][i]] == [_bits(v) for v in r["nsd"]], (kind, s["nsd"][i], r["nsd"])
        assert s["sel"][i, :, 0].tolist() == [list(p[0]) for p in r["sel"]] and s["within"][i].tolist() == [list(w) for w in r["within"]]
    assert math.isnan(s["hd_pct"][2, 0]) and s["nsd"][2].tolist() == [0.0, 0.0] and math.isnan(s["nsd"][4, 0]) and s["nsd"][5].tolist() == [1.0, 1.0]


def test_the_evaluators_csv_gains_columns_only_when_asked(tmp_path):
    from ultrasound_modeling_amd import TBIEvaluator as E
    rng = np.random.default_rng(5)
    prob = rng.random((3, 16, 24)).astype(np.float32)
    label = np.kron(rng.choice([0.0, 1.0, 2.0], size=(3, 4, 6), p=[0.5, 0.2, 0.3]), np.ones((4, 4)))
    label[2] = 0.0                                                                                              # an image without a labelled bleed
    res = E.PolarResult(prob, prob, None, label, np.zeros_like(prob), np.asarray(["u", "v", "w"]))
    assert E.write_surface_csv(tmp_path / "old.csv", res, device=DEV) == 3
    assert E.write_surface_csv(tmp_path / "new.csv", res, device=DEV, percentiles=(95,), tolerances=(2,)) == 3
    old = list(csv.reader(open(tmp_path / "old.csv")))
    new = list(csv.reader(open(tmp_path / "new.csv")))
    assert old[0] == ["name", "hd", "assd", "n_pred", "n_label"] and new[0] == old[0] + ["hd95", "hd95_directed", "nsd2"]
    for i in range(3):
        assert new[1 + i][:5] == old[1 + i]
        r = SR.scores(prob[i] > 0.5, label[i] > 1.5, (95,), (2,))
        assert new[1 + i][5:] == [repr(r["pooled"][0]), repr(r["directed"][0]), repr(r["nsd"][0])]
    assert new[3][5:7] == ["nan", "nan"] and new[3][7] == "0.0"


def _raw(n, h, w, c, seed):
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, 1, h, w, c + 2), dtype=np.float64)          # label, c displacement channels, bMode (Dataset_2.py:33-43)
    raw[..., 1:c + 1] = np.clip(rng.standard_normal((n, 1, h, w, c)) * 0.3, -1, 1)
    raw[..., 0] = np.kron(rng.choice([0.0, 1.0, 1.3, 1.5, 2.0], size=(n, 1, h // 8, w // 8), p=[0.5, 0.2, 0.1, 0.1, 0.1]), np.ones((8, 8)))
    return raw


class _Recorder:
    def __init__(self, net):
        self.net, self.test = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def step(self, x, y, **kw):
        out = self.net.step(x, y, **kw)
        self.test.append((torch.as_tensor(y).float().cpu().numpy().copy(), out[-1].float().cpu().numpy().copy()))
        return out


def test_mainnumpy_process_scores_the_validation_set(monkeypatch):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.Dataset_2 import Dataset
    from ultrasound_modeling_amd.MainNumpy import Process
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    raw = _raw(6, 64, 64, 10, seed=1)
    ds = Dataset(train_data=raw, val_data=raw[:3], num_classes=3)
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=10, learning_rate=1e-3)
    random.seed(0)
    rec = _Recorder(net)
    proc = Process(batch_size=2, num_classes=3, surface=dict(percentiles=[95, 100], tolerances=[2]))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        proc.test(rec, ds, epoch=1)
    torch.cuda.synchronize()
    with_surface = buf.getvalue().splitlines()
    h = proc.history[-1]
    y = np.concatenate([t[0] for t in rec.test])
    p = np.concatenate([t[1] for t in rec.test])
    n = y.shape[0]                                          # 2: a validation set shorter than next_test's 16 comes back without its last image
    assert n == 2 == h["surface_images"]
    rows = [SR.scores(p[i][..., :3].argmax(-1) == 2, y[i][..., 2] > 0.5, (95, 100), (2,)) for i in range(n)]
    ok = [r for r in rows if not math.isnan(r["pooled"][0])]
    ok_nsd = [r for r in rows if not math.isnan(r["nsd"][0])]
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    want = {"surface_hd_pct": [mean([r["pooled"][k] for r in ok]) for k in range(2)],
            "surface_hd_pct_directed": [mean([r["directed"][k] for r in ok]) for k in range(2)], "surface_nsd": [mean([r["nsd"][0] for r in ok_nsd])],
            "surface_scored": len(ok), "surface_nsd_scored": len(ok_nsd), "surface_images": n}
    for k, v in want.items():
        got = h[k]
        assert ([_bits(x) for x in got] == [_bits(x) for x in v]) if isinstance(v, list) else got == v, (k, got, v)
    line = [l for l in with_surface if l.startswith("surface")]
    assert len(line) == 1 and with_surface.index(line[0]) == len(with_surface) - 1
    assert line[0] == ("surface (mean over scored images): hd95 = {}, hd95_directed = {}, hd100 = {}, hd100_directed = {}, nsd2 = {} "
                       "({} of 2 images have both surfaces, {} at least one)").format(
        want["surface_hd_pct"][0], want["surface_hd_pct_directed"][0], want["surface_hd_pct"][1], want["surface_hd_pct_directed"][1],
        want["surface_nsd"][0], len(ok), len(ok_nsd))
    # without surface=: the parent's lines and keys, and no surface kernel
    def boom(*a, **k):
        raise AssertionError("surface_stats launched without surface=")
    monkeypatch.setattr(ops, "surface_stats", boom)
    ds.reset_idx()
    plain = Process(batch_size=2, num_classes=3)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        plain.test(net, ds, epoch=1)
    what = lambda lines: [l.split(" = ")[0] for l in lines]                 # (the values after "=" come from another run of the step)
    assert what(buf.getvalue().splitlines()) == what(with_surface[:-1]) == ["", "Test...", "loss", "IoU", "f1", "precision", "recall"]
    assert set(plain.history[-1]) == set(h) - set(want) == {"precision", "recall", "f1", "c2_precision", "c2_recall", "c2_f1", "mean_iou", "phase", "epoch",
                                                           "loss"}
