"""GPU tests of the elastic / affine warp of training batches (csrc/warp.hip).

Shapes (B, H, W, C, sigma): odd sizes; a radius (10) beyond W and most of H; the real width and channel count at radius 32 (three column tiles,
two row tiles, more than one workgroup of the gather); and radius 0, the identity smoothing.  Every shape runs with fp32 and fp64 ``x``, an
inactive sample that holds a NaN with a payload and an Inf, and affines that push part of the image outside.

Everything is BITWISE: against the NumPy restatement (tests/warp_restatement.py, itself pinned to SciPy in tests/test_cpu_warp.py), against
slices and ``torch.flip`` for the warps that have a closed form, eager against HIP-graph replay, ``next_train`` against ``dataAug_batch`` of the
restated warp, and two ranks against one."""
import functools
import math
import random

import numpy as np
import pytest
import torch

import warp_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 37, 19, 3, 3.0), (2, 16, 5, 1, 2.5), (2, 64, 80, 10, 8.0), (2, 9, 7, 2, 0.1)]
DTYPES = [np.float32, np.float64]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b):
    a, b = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _diff(a, b):
    a, b = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (a, b))
    return f"{int((_bits(a) != _bits(b)).sum())} of {a.size} elements differ"


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Inputs, draws, weights and an injected field of one shape; the LAST sample is inactive and holds a NaN with a payload and an Inf."""
    from ultrasound_modeling_amd import warp as Wp
    B, H, W, Cc, sigma = shape
    rng = np.random.default_rng(B * 1000 + H)
    x = rng.standard_normal((B, H, W, Cc)).astype(dtype)
    y = (rng.integers(0, 3, (B, H, W)) + rng.random((B, H, W)) * 0.04).astype(np.float32)
    nan = np.array([0x7FC12345], np.int32).view(np.float32)[0] if dtype == np.float32 else np.array([0x7FF8000000012345], np.int64).view(np.float64)[0]
    x[B - 1, 1, 2, 0], x[B - 1, H - 1, W - 1, Cc - 1], x[B - 1, 0, 0, 0] = nan, np.inf, -0.0
    y[B - 1, 2, 1], y[B - 1, 0, 0] = np.array([0x7FC00077], np.int32).view(np.float32)[0], -np.inf
    cfg = Wp.warp_config({"sigma": sigma, "magnitude": (2.0, 1.0)})
    params = []
    for b in range(B):
        theta, ls, sh = ((9.0, math.log(1.1), (1.25, -0.75)), (-6.0, -0.08, (-2.5, 1.5)), (3.0, 0.0, (0.0, 0.0)))[b % 3]
        params.append({"active": b != B - 1, "seed": 0x1234567 * (b + 1) + (1 << 62) * (b % 2), "alpha": Wp.alpha_of(cfg),
                       "aff": Wp.affine_of(theta, ls, sh, H, W)})
    fld = rng.uniform(-1, 1, (B, 2, H, W))
    return x, y, params, Wp.gaussian_weights(sigma), fld


@functools.lru_cache(maxsize=None)
def _restated(shape, dtype, injected):
    x, y, params, w, fld = _case(shape, dtype)
    return R.warp(x, y, params, w, fld if injected else None)


def _run(x, y, params, w, fld=None, want_debug=True):
    from ultrasound_modeling_amd import warp as Wp
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = Wp.elastic_warp(xd, yd, Wp.sample_table(params, DEV), torch.from_numpy(w).to(DEV), field=None if fld is None else torch.from_numpy(fld).to(DEV),
                          want_debug=want_debug)
    torch.cuda.synchronize()
    assert _same(xd, x) and _same(yd, y), "the inputs were modified"
    return out


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_injected_field_equals_the_restatement_bit_for_bit(shape, dtype):
    x, y, params, w, fld = _case(shape, dtype)
    assert len(w) - 1 == int(4 * shape[4] + 0.5)
    xo, yo, disp, used = _run(x, y, params, w, fld)
    rx, ry, rd, ru = _restated(shape, dtype, True)
    outside = float((rx[:-1] == 0).all(-1).mean())
    assert 0.02 < outside < 0.6, outside                               # part of every active image samples outside
    assert _same(used, ru), "field_out: " + _diff(used, ru)
    assert _same(disp, rd), "disp_out: " + _diff(disp, rd)
    assert _same(yo, ry), "y_out: " + _diff(yo, ry)
    assert _same(xo, rx), "x_out: " + _diff(xo, rx)
    B = shape[0]
    assert _same(xo[B - 1], x[B - 1]) and _same(yo[B - 1], y[B - 1])   # the inactive sample: a copy, NaN payload and Inf included
    assert not disp[B - 1].any() and not used[B - 1].any()
    xo2, yo2 = _run(x, y, params, w, fld, want_debug=False)            # the optional outputs change nothing
    assert _same(xo2, xo) and _same(yo2, yo)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_generated_field_equals_the_restated_hash_bit_for_bit(shape, dtype):
    x, y, params, w, _ = _case(shape, dtype)
    xo, yo, disp, used = _run(x, y, params, w)
    rx, ry, rd, ru = _restated(shape, dtype, False)
    for b, p in enumerate(params[:-1]):
        assert _same(used[b], R.field(p["seed"], shape[1], shape[2])), f"sample {b}: " + _diff(used[b], ru[b])
    assert _same(used, ru) and _same(disp, rd) and _same(yo, ry) and _same(xo, rx), _diff(xo, rx)
    if shape[4] >= 2.5:
        assert float(np.abs(rd[0]).max()) > 0.5                        # the warp is not a no-op


# ------------------------------------------------------------------------------------------------ checks that do not rest on the restatement
def _plain(shape, dtype, aff, active=True):
    from ultrasound_modeling_amd import warp as Wp
    x, y, _, w, _ = _case(shape, dtype)
    x, y = x[:-1], y[:-1]                                              # the finite samples
    params = [{"active": active, "seed": 5 + b, "alpha": (0.0, 0.0), "aff": aff} for b in range(x.shape[0])]
    xo, yo = _run(x, y, params, w, want_debug=False)
    return x, y, xo.cpu().numpy(), yo.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_integer_translation_is_the_shifted_slice(shape, dtype):
    x, y, xo, yo = _plain(shape, dtype, [1.0, 0.0, 0.0, 1.0, 2.0, -3.0])       # out[i, j] = in[i + 2, j - 3]
    H, W = shape[1], shape[2]
    wx, wy = np.zeros_like(x), np.zeros_like(y)
    wx[:, :H - 2, 3:], wy[:, :H - 2, 3:] = x[:, 2:, :W - 3], y[:, 2:, :W - 3]
    assert np.array_equal(xo, wx) and np.array_equal(yo, wy)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mirror_is_torch_flip(shape, dtype):
    x, y, xo, yo = _plain(shape, dtype, [1.0, 0.0, 0.0, -1.0, 0.0, float(shape[2] - 1)])
    assert np.array_equal(xo, torch.flip(torch.from_numpy(x), dims=[2]).numpy()) and np.array_equal(yo, torch.flip(torch.from_numpy(y), dims=[2]).numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_labels_are_never_interpolated_and_the_image_stays_in_range(shape, dtype):
    x, y, params, w, _ = _case(shape, dtype)
    x, y, params = x[:-1], y[:-1], params[:-1]
    xo, yo = (t.cpu().numpy() for t in _run(x, y, params, w, want_debug=False))
    for b in range(x.shape[0]):
        assert set(np.unique(yo[b])) <= set(np.unique(y[b])) | {np.float32(0)}
        assert xo[b].min() >= min(0.0, x[b].min()) and xo[b].max() <= max(0.0, x[b].max())
        assert not np.array_equal(xo[b], x[b])


# ------------------------------------------------------------------------------------------------ graph capture
def test_eager_runs_and_a_graph_replay_give_the_same_bits_and_follow_the_table():
    from ultrasound_modeling_amd import warp as Wp
    shape = SHAPES[0]
    x, y, params, w, _ = _case(shape, np.float64)
    xd, yd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(w).to(DEV)
    table = Wp.sample_table(params, DEV)
    e1 = Wp.elastic_warp(xd, yd, table, wd)
    e2 = Wp.elastic_warp(xd, yd, table, wd)
    assert _same(e1[0], e2[0]) and _same(e1[1], e2[1])
    xo, yo = torch.empty_like(xd), torch.empty_like(yd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Wp.elastic_warp(xd, yd, table, wd, out=(xo, yo))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # a single stream; nothing in the call synchronises or allocates outside torch's pool
        Wp.elastic_warp(xd, yd, table, wd, out=(xo, yo))
    xo.zero_(), yo.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(xo, e1[0]) and _same(yo, e1[1])
    # other draws in the SAME device table: the next replay follows them without a recapture
    other = [dict(p, active=b != 0, seed=p["seed"] + 99, aff=params[(b + 1) % len(params)]["aff"]) for b, p in enumerate(params)]
    x2 = x.copy()
    x2[-1] = np.nan_to_num(x2[-1], nan=0.5, posinf=1.0)               # the sample that becomes active must be finite for the comparison below
    xd.copy_(torch.from_numpy(x2))
    y2 = np.nan_to_num(y, nan=1.0, neginf=2.0)
    yd.copy_(torch.from_numpy(y2))
    table.copy_(Wp.sample_table(other, DEV))
    graph.replay()
    torch.cuda.synchronize()
    rx, ry, _, _ = R.warp(x2, y2, other, w)
    assert _same(xo, rx) and _same(yo, ry), _diff(xo, rx)
    assert not _same(xo, e1[0])


# ------------------------------------------------------------------------------------------------ the datasets
def _raw(n=5, h=12, w=10, seed=4):
    rng = np.random.default_rng(seed)
    raw = rng.random((n, 1, h, w, 12))
    raw[..., 0] = rng.integers(0, 3, (n, 1, h, w)) * (rng.random((n, 1, h, w)) > 0.3)      # labels 0 / 1 / 2 with holes for imageReduc
    return raw


CFG = {"sigma": 1.5, "magnitude": (1.5, 1.0), "p": 0.6, "rotate": 8.0, "scale": 0.1, "shift": (1.0, 0.5)}


def test_next_train_is_dataaug_of_the_restated_warp():
    from ultrasound_modeling_amd import DataAugs, Dataset_2, warp as Wp
    raw, B = _raw(), 4
    params = [DataAugs.draw(random.Random(30 + i)) for i in range(B)]
    ds = Dataset_2.Dataset(train_data=raw, val_data=raw[:2], warp=CFG, warp_seed=17)
    rw = random.Random(17)
    wp = [Wp.draw_warp(rw, Wp.warp_config(CFG), 12, 10) for _ in range(B)]
    assert any(p["active"] for p in wp) and not all(p["active"] for p in wp)
    x0, y0 = ds.x_tr[:B].cpu().numpy(), ds.y_tr[:B].cpu().numpy()
    rx, ry, rd, _ = R.warp(x0, y0, wp, Wp.gaussian_weights(1.5))
    assert float(np.abs(rd).max()) > 0.5 and not np.array_equal(ry, y0)
    want = DataAugs.dataAug_batch(torch.from_numpy(rx).to(DEV), torch.from_numpy(ry).to(DEV), params=params, num_classes=3)
    got = ds.next_train(B, params=params)
    assert _same(got[0].view(torch.int16), want[0].view(torch.int16)) and _same(got[1], want[1]) and got[2] is False
    assert _same(ds.x_tr[:B], x0) and _same(ds.y_tr[:B], y0)          # the resident training set is not modified
    # without warp, and with a warp that never fires: today's next_train, bit for bit
    today = DataAugs.dataAug_batch(ds.x_tr[:B], ds.y_tr[:B], params=params, num_classes=3)
    assert not _same(today[1], want[1])
    for kw in (dict(), dict(warp=dict(CFG, p=0.0), warp_seed=17)):
        d2 = Dataset_2.Dataset(train_data=raw, val_data=raw[:2], **kw)
        out = d2.next_train(B, params=params)
        assert _same(out[0].view(torch.int16), today[0].view(torch.int16)) and _same(out[1], today[1]), kw
    xt, yt, _ = ds.next_test(2)                                       # validation batches are never warped
    xp, yp, _ = Dataset_2.Dataset(train_data=raw, val_data=raw[:2]).next_test(2)
    assert _same(xt.view(torch.int16), xp.view(torch.int16)) and _same(yt, yp)


@pytest.mark.parametrize("noise", [False, True], ids=["no-noise", "reference-draws"])
def test_two_ranks_concatenated_equal_one(noise):
    """World 2 against world 1, global batches of 4 and 3.  ``usseg_augment`` (unchanged here) seeds the noise of a pixel with its index in the
    LAUNCHED batch, so a sample that sits at another position in its rank's launch than in the world-1 launch gets other noise - with and without
    a warp.  With noise-free draws the ranks' slices concatenated are the world-1 batch bit for bit; with the reference's draws the labels are, and
    the image of every sample that has no noise or keeps its position (rank 0's) is."""
    from ultrasound_modeling_amd import DataAugs
    from ultrasound_modeling_amd.Dataset import Dataset

    class _Quiet(Dataset):
        draw = staticmethod(lambda rng=random: dict(DataAugs.draw(rng), noise=False))
    cls = Dataset if noise else _Quiet
    raw = _raw(7, 48, 20)                                              # room for the reference's shifts (up to 30 x 12) and clip boxes
    runs = []
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        ds = cls(train_data=raw, val_data=raw[:2], batch_size=4, warp=CFG, warp_seed=23)
        runs.append(list(ds.train_batches(rank, world, rng=random.Random(7))))
    plain = list(cls(train_data=raw, val_data=raw[:2], batch_size=4).train_batches(rng=random.Random(7)))
    rng = random.Random(7)
    noisy = [DataAugs.draw(rng)["noise"] and noise for _ in range(7)]
    assert [b for _, _, b in runs[0]] == [4, 3]
    compared = 0
    for i, (x, y, b) in enumerate(runs[0]):
        parts = [r[i] for r in runs[1:] if r[i][0] is not None]
        assert sum(p[0].shape[0] for p in parts) == b and parts[0][0].shape[0] == 2
        xs, ys = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        assert _same(ys, y), _diff(ys, y)
        for s in range(b):
            if s < 2 or not noisy[4 * i + s]:
                assert _same(xs[s].view(torch.int16), x[s].view(torch.int16)), (i, s)
                compared += 1
    assert any(not _same(plain[i][1], runs[0][i][1]) for i in range(2))   # and the warp did something
    assert compared == (4 if noise else 7)                            # these seeds: every sample of rank 1 draws noise
