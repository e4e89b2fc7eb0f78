"""Threshold sweeps and temperature scaling on the GPU: the three kernels of csrc/operating_point.hip against the NumPy restatement
(tests/operating_point_restatement.py), and ``fit_temperature`` / ``Cascade(temperature=)`` / ``Process(sweep=)`` against the same computation
composed of public calls.

Bounds.  The sweep counters, and the valid / invalid counts of the NLL, are integers and equal exactly.  An NLL sum lies within the sum over
its valid pixels of ``R.nll_pixel_bound`` (its docstring counts the fp32 roundings per pixel and their magnitudes, half a quantisation unit,
and the error of the device's logf / expf) of the fp64 restatement's sum.  No documented error of those two functions ships with the toolchain,
so they were measured against fp64 over the arguments these tests feed them (``tools/time_sweep.py --probe``: logf at most 2.1845 ulp over
1 010 574 distinct arguments in [1e-7, 4], expf at most 0.8298 ulp over 2 359 008 in [-257.9, 0]) and the bound takes four
times the largest error seen: L = 8.738, X = 3.3192.  The applied probabilities are bounded per
element by ``route_probe.assert_elementwise`` with u = 2^-24, mag = the restated probability and the project's fp32 constant for a C-term
sum.  Each test prints the largest error it saw in the bound's units (``pytest -s`` shows them; DESIGN.md section 8 records them)."""
import numpy as np
import pytest
import torch

import operating_point_restatement as R
from route_probe import assert_elementwise, c_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
L_ULP, X_ULP = 4 * 2.1845, 4 * 0.8298        # four times the largest logf / expf error measured (module docstring)
# (B, H, W, C, base offset in floats): test_gpu_ensemble's shapes with its 16-byte-offset variant, and 66 560 pixels - more than the 65 536 one
# trip of the capped grid covers, so the grid-stride loop runs a second, partial trip
SHAPES = [(2, 5, 7, 3, 0), (1, 4, 8, 3, 0), (3, 2, 4, 2, 0), (1, 3, 5, 4, 0), (2, 5, 7, 3, 1), (1, 260, 256, 3, 0)]
IDS = ["odd-w-tail", "pure-vector", "two-classes", "four-classes", "offset-generic", "second-trip"]


@pytest.fixture(autouse=True)
def _default_fusion(monkeypatch):
    """The product defaults (folded inference BatchNorm, fused stem and cardinal launches), whatever an earlier test left in the modules."""
    import ultrasound_modeling_amd.Decoder as D
    import ultrasound_modeling_amd.ResNest as Rn
    for mod, name in ((D, "_FOLD_BN"), (Rn, "_FOLD_BN"), (Rn, "_FUSED_STEM"), (Rn, "_FUSED_CARDINAL")):
        monkeypatch.setattr(mod, name, True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit-for-bit equality (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev(a, off=0):
    """A contiguous device tensor of a's values whose base is `off` floats past a 16-byte aligned address."""
    a = torch.as_tensor(np.array(a)) if isinstance(a, np.ndarray) else torch.as_tensor(a)      # (a copy: the shared cases are read-only)
    buf = torch.empty(a.numel() + 4, dtype=a.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.numel()].view(a.shape)
    v.copy_(a)
    return v


_CASES = {}


def _case(B, H, W, C):
    """Softmax probabilities with exact 0 and exact 1, scores exactly on bin edges, one NaN pixel, one pixel above 1 and one negative; one-hot
    labels with one soft pixel.  Computed once per shape and never modified."""
    key = (B, H, W, C)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * B + H * W + C)
        z = rng.standard_normal((B, H, W, C)) * 3
        e = np.exp(z - z.max(-1, keepdims=True))
        probs = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        flat = probs.reshape(-1, C)
        M = len(flat)
        flat[0] = np.eye(C, dtype=np.float32)[C - 1]             # exact zeros and an exact one in the last class
        flat[3 % M] = np.eye(C, dtype=np.float32)[0]
        flat[5 % M] = 1.0 / C if C != 3 else 0.25                # C = 2, 4: exactly on an edge of every bins >= 4; C = 3: 0.25 each (sums to 0.75)
        flat[6 % M, :] = 0.5 if C == 2 else (np.array([0.5, 0.25, 0.25, 0.0][:C], np.float32))
        flat[7 % M, C - 1] = np.float32(0.015625)                # 1/64
        flat[9 % M] = np.nan                                      # invalid under every cls
        flat[10 % M] = 1.5                                        # above 1
        flat[12 % M, 0] = -0.25                                   # negative: invalid for cls 0 and for the temperature
        y = np.eye(C, dtype=np.float32)[rng.integers(0, C, (B, H, W))]
        y.reshape(-1, C)[8 % M] = 0.5                             # a soft label: the first maximum is class 0
        probs.setflags(write=False)
        y.setflags(write=False)
        _CASES[key] = (probs, y)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_score_sweep_equals_the_restatement_exactly(shape):
    from ultrasound_modeling_amd import ops
    B, H, W, C, off = shape
    probs, y = _case(B, H, W, C)
    pd, yd = _dev(probs, off), _dev(y, off)
    M = B * H * W
    for bins in (2, 64, 4096):
        for cls in range(C):
            counts = torch.zeros(2 * bins + 1, dtype=torch.int64, device=DEV)
            ops.score_sweep(pd, yd, counts, bins, cls)
            once = counts.cpu().numpy().copy()
            ops.score_sweep(pd, yd, counts, bins, cls - C)                       # a negative cls counts from the last class
            twice = counts.cpu().numpy()
            ref = R.sweep_counts(probs, y, bins, cls)
            what = f"score_sweep {shape} bins={bins} cls={cls}"
            assert np.array_equal(once, ref), what
            assert once.sum() == M and once[2 * bins] >= 2, what                # every pixel is counted once; the NaN and the 1.5 are invalid
            assert np.array_equal(twice, 2 * once), what                        # ADDED INTO


def test_score_sweep_of_an_empty_batch_launches_nothing():
    from ultrasound_modeling_amd import ops
    counts = torch.arange(129, dtype=torch.int64, device=DEV)
    empty = torch.empty((0, 4, 4, 3), dtype=torch.float32, device=DEV)
    ops.score_sweep(empty, empty, counts, 64, 2)
    assert torch.equal(counts.cpu(), torch.arange(129))


@pytest.mark.parametrize("odd", ["none", "lane-17", "first-lane", "first-lane-invalid", "label-of-lane-40"])
def test_score_sweep_wave_aggregated_path_counts_exactly(odd):
    """640 pixels = ten waves in three workgroups, every pixel in one bin with one label - the wave adds its population count once - and the
    inputs that must leave that path: one lane per wave differs (in the middle, or the wave's first lane: the lane whose key is broadcast),
    the first lane holds no key at all (an invalid score: the first ACTIVE lane is lane 1), or one lane differs in its label alone."""
    from ultrasound_modeling_amd import ops
    probs = np.empty((2, 8, 40, 3), np.float32)
    probs[...] = (0.9, 0.0625, 0.0375)
    y = np.zeros_like(probs)
    y[..., 0] = 1
    fp, fy = probs.reshape(-1, 3), y.reshape(-1, 3)
    lanes = np.arange(len(fp)) % 64
    if odd == "lane-17":
        fp[lanes == 17] = (0.1, 0.1, 0.8)
    elif odd == "first-lane":
        fp[lanes == 0] = (0.1, 0.1, 0.8)
    elif odd == "first-lane-invalid":
        fp[lanes == 0] = np.nan
    elif odd == "label-of-lane-40":
        fy[lanes == 40] = (0, 0, 1)
    pd, yd = _dev(probs), _dev(y)
    for bins in (2, 64, 4096):
        for cls in (0, 2):
            counts = torch.zeros(2 * bins + 1, dtype=torch.int64, device=DEV)
            ops.score_sweep(pd, yd, counts, bins, cls)
            got = counts.cpu().numpy()
            assert np.array_equal(got, R.sweep_counts(probs, y, bins, cls)), (odd, bins, cls)
            assert got.sum() == 640 and np.count_nonzero(got) == (1 if odd == "none" else 2)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_thresholds_reproduce_the_device_counts_on_the_host(shape):
    """``probs[..., cls] > threshold[k]`` over the valid pixels is the device's tp + fp at k, for every k: the returned threshold can go to
    every ``threshold=`` argument as it is."""
    from ultrasound_modeling_amd import metrics
    B, H, W, C, off = shape
    probs, y = _case(B, H, W, C)
    bins = 64 if B * H * W > 1000 else 4096
    for cls in range(C):
        sw = metrics.SweepCounts(bins, cls, device=DEV)
        sw.update(_dev(probs, off), _dev(y, off))
        r = sw.result()
        s = probs.reshape(-1, C)[:, cls]
        with np.errstate(invalid="ignore"):
            s = s[(s >= 0) & (s <= 1)]
        assert len(s) + r["n_invalid"] == B * H * W
        above = np.array([int((s > t).sum()) for t in r["threshold"]])
        assert np.array_equal(above, r["tp"] + r["fp"]), (shape, cls)
        want = R.sweep_from_counts(R.sweep_counts(probs, y, bins, cls))
        assert r["auc"] == want["auc"] and r["best_dice"] == want["best_dice"] and r["average_precision"] == want["average_precision"]
        sw.reset()
        assert not bool(sw.counts.any())


def test_score_sweep_in_a_captured_graph_equals_eager():
    from ultrasound_modeling_amd import ops
    probs, y = _case(2, 5, 7, 3)
    pd, yd = _dev(probs), _dev(y)
    eager = torch.zeros(129, dtype=torch.int64, device=DEV)
    ops.score_sweep(pd, yd, eager, 64, 2)
    counts = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.score_sweep(pd, yd, counts, 64, 2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    counts.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.score_sweep(pd, yd, counts, 64, 2)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(counts, 2 * eager)


# ------------------------------------------------------------------------------------------------ the NLL of the candidates
BETAS16 = [float(np.float32(0.125 * (64.0 ** (i / 15)))) for i in range(16)]          # round 0 of the fit: 1/8 .. 8


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_temperature_nll_is_within_the_derived_bound_and_reproducible(shape):
    from ultrasound_modeling_amd import ops
    B, H, W, C, off = shape
    probs, y = _case(B, H, W, C)
    pd, yd = _dev(probs, off), _dev(y, off)
    shared = BETAS16[9]
    got = {}
    for betas in ([shared], [shared, 16.0], BETAS16):
        counts = torch.zeros(len(betas) + 2, dtype=torch.int64, device=DEV)
        ops.temperature_nll(pd, yd, betas, counts)
        again = torch.zeros_like(counts)
        ops.temperature_nll(pd, yd, betas, again)
        assert torch.equal(counts, again)                                          # two identical calls: bit-identical
        ops.temperature_nll(pd, yd, betas, again)
        assert torch.equal(again, 2 * counts)                                      # ADDED INTO
        c = counts.cpu().numpy()
        ref, T, n_valid, n_invalid = R.nll(probs, y, betas)
        what = f"temperature_nll {shape} n_beta={len(betas)}"
        assert c[len(betas)] == n_valid and c[len(betas) + 1] == n_invalid and n_invalid >= 3 and n_valid + n_invalid == B * H * W, what
        worst = 0.0
        for j, beta in enumerate(betas):
            bound = float(R.nll_pixel_bound(T[:, j], beta, C, L_ULP, X_ULP).sum())
            err = abs(float(c[j]) - float(ref[:, j].sum() * R.UNIT))
            worst = max(worst, err / bound)
            assert err <= bound, f"{what} beta={beta}: off by {err:.1f} counts, bound {bound:.1f}"
        print(f"{what}: largest error {worst:.4f} of the bound")
        got[len(betas)] = c
    assert got[1][0] == got[2][0] == got[16][9]                                    # a shared beta: the same counter whatever travels with it


def test_temperature_nll_of_an_empty_batch_launches_nothing():
    from ultrasound_modeling_amd import ops
    counts = torch.arange(4, dtype=torch.int64, device=DEV)
    empty = torch.empty((0, 4, 4, 3), dtype=torch.float32, device=DEV)
    ops.temperature_nll(empty, empty, [0.5, 2.0], counts)
    assert counts.cpu().tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ applying a temperature
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_temperature_is_bounded_per_element_and_safe_in_place(shape):
    from ultrasound_modeling_amd import ops
    B, H, W, C, off = shape
    probs, _ = _case(B, H, W, C)
    pd = _dev(probs, off)
    flat = probs.reshape(-1, C)
    top2 = np.sort(np.nan_to_num(flat, nan=0.0), -1)
    decided = (top2[:, -1] - top2[:, -2] > 1e-6) if C > 1 else np.ones(len(flat), bool)
    for beta in (0.5, 1.0, 2.5):
        bd = torch.full((1,), beta, dtype=torch.float32, device=DEV)
        out = ops.apply_temperature(pd, bd)
        torch.cuda.synchronize()
        assert out.data_ptr() != pd.data_ptr() and _same(pd.cpu(), torch.from_numpy(np.array(probs)))       # the input is left alone
        ref = R.apply_temperature(probs, beta)
        got = out.cpu().numpy()
        nan = np.isnan(ref)
        what = f"apply_temperature {shape} beta={beta}"
        assert np.array_equal(np.isnan(got), nan) and nan.reshape(-1, C).all(-1).sum() >= 1, what      # the NaN pixels match, all classes of each
        g, r = np.where(nan, 0.0, got), np.where(nan, 0.0, ref)
        has = r > 0
        print(f"{what}: largest error {float((np.abs(g - r)[has] / (U * r[has])).max()):.3f} u*mag, {float(np.abs(g - r).max()):.3g} absolute")
        assert_elementwise(torch.from_numpy(g), torch.from_numpy(r), torch.from_numpy(r), U, c_f32(C), what=what)
        sums = got.astype(np.float64).sum(-1).reshape(-1)[~nan.reshape(-1, C).any(-1)]
        assert np.abs(sums - 1).max() <= C * 2.0 ** -23, what                              # each pixel sums to 1 within C ulp
        ok = decided & ~nan.reshape(-1, C).any(-1)
        assert np.array_equal(got.reshape(-1, C)[ok].argmax(-1), np.nan_to_num(flat, nan=0.0)[ok].argmax(-1)), what
        inplace = pd.clone() if off == 0 else _dev(probs, off)
        assert ops.apply_temperature(inplace, bd, out=inplace).data_ptr() == inplace.data_ptr()
        assert _same(inplace, out), what                                                   # out aliasing probs: the same bits
        if off:                                                                            # the generic path equals the float4 path
            assert _same(ops.apply_temperature(_dev(probs, 0), bd), out), what


# ------------------------------------------------------------------------------------------------ the fit
def _fit_case(factor, seed=7):
    rng = np.random.default_rng(seed)
    z = 2 * rng.standard_normal((2, 8, 6, 3))
    e = np.exp(z - z.max(-1, keepdims=True))
    true = e / e.sum(-1, keepdims=True)
    lab = np.array([rng.choice(3, p=p) for p in true.reshape(-1, 3)]).reshape(2, 8, 6)
    zf = factor * z
    e = np.exp(zf - zf.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), np.eye(3, dtype=np.float32)[lab]


@pytest.mark.parametrize("factor", [0.5, 1.0, 2.5])
def test_fit_temperature_is_the_restated_search_on_the_device_counters(factor):
    from ultrasound_modeling_amd import metrics, ops
    probs, y = _fit_case(factor)
    batches = [(_dev(probs[:1]), _dev(y[:1])), (probs[1:], y[1:])]                 # two batches: a device pair and a numpy pair
    fit = metrics.fit_temperature(batches, device=DEV)
    again = metrics.fit_temperature(batches, device=DEV)
    assert fit == again                                                            # integers all the way: bitwise reproducible
    pd, yd = _dev(probs), _dev(y)

    def evaluate(betas):
        counts = torch.zeros(len(betas) + 2, dtype=torch.int64, device=DEV)
        ops.temperature_nll(pd, yd, betas, counts)
        return counts.cpu().tolist()
    beta, best, at1, spacing = R.search(evaluate)
    dense = R.dense_search(probs, y)
    print(f"factor {factor}: beta {fit['beta']:.5f}, dense fp64 {dense:.5f}, final spacing {spacing:.2e}")
    assert fit["beta"] == beta and abs(beta - dense) <= spacing
    assert fit["n"] == 96 and fit["n_invalid"] == 0 and fit["temperature"] == 1.0 / beta
    assert fit["nll"] == best * (2.0 ** -20 / 96) and fit["nll_at_1"] == at1 * (2.0 ** -20 / 96) and fit["nll"] <= fit["nll_at_1"]
    assert fit["bracket"][0] <= beta <= fit["bracket"][1] or beta == 1.0
    with pytest.raises(ValueError, match="upper edge"):
        metrics.fit_temperature(batches, hi=0.25, device=DEV)


# ------------------------------------------------------------------------------------------------ the cascade
def _arch_b(classes=3, cin=1, seed=3, img=(64, 64)):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    return VisionTransformer(2, img, classes, in_channels=cin, seed=seed)


def _x(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, C, generator=g).to(DEV)


def _split_gate(mask_model, x):
    """Shift the mask model's class-0 head bias so that about half the pixels of x are gated (a random model gates all or none)."""
    p0 = mask_model.predict(x)[..., 0].double()
    med = p0.median().item()
    mask_model.decoder.head.bias.data[0] -= float(np.log(med / (1 - med)))
    mask_model.repack()


@pytest.fixture(scope="module")
def models():
    bleed, mask = _arch_b(3, cin=10, seed=3), _arch_b(2, cin=10, seed=4)
    x = _x(2, 64, 64, 10, seed=50)
    _split_gate(mask, x)
    return bleed, mask, x


def _beta(T):
    return torch.full((1,), 1.0 / T, dtype=torch.float32, device=DEV)


def test_cascade_without_a_temperature_adds_no_launch_and_with_one_applies_it(models, monkeypatch):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.TBIEvaluator import Cascade, CascadeOutput
    bleed, mask, x = models
    real = ops.apply_temperature

    def boom(*a, **k):
        raise AssertionError("apply_temperature launched without a temperature")
    monkeypatch.setattr(ops, "apply_temperature", boom)
    c0 = Cascade(bleed, mask)
    assert c0.temperature is None
    plain = tuple(t.clone() for t in c0.predict(x))
    monkeypatch.setattr(ops, "apply_temperature", real)
    # today's cascade, composed of public calls: the gate applied on the host, the bleed model, the maps
    assert 0.05 < plain[1].double().mean().item() < 0.95
    xg = x.clone()
    xg[plain[1].bool()] = 0
    want = bleed.predict(xg).clone()
    pm, bp = ops.cascade_maps(want)
    assert _same(plain[0], want) and _same(plain[2], pm) and _same(plain[3], bp)
    for T in (2.0, 0.75):
        c = Cascade(bleed, mask, temperature=T)
        assert c.temperature == 1.0 / float(np.float32(1.0 / T))
        out = c.predict(x)
        assert isinstance(out, CascadeOutput) and torch.equal(out.mask, plain[1])
        scaled = ops.apply_temperature(plain[0], _beta(T))
        pm, bp = ops.cascade_maps(scaled)
        assert _same(out.probs, scaled) and _same(out.prob_map, pm) and _same(out.bleed_prob, bp)
        assert not _same(out.probs, plain[0])
    with pytest.raises(ValueError, match="temperature"):
        Cascade(bleed, mask, temperature=0.0)


def test_cascade_temperature_reaches_a_captured_graph_without_a_recapture(models):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.TBIEvaluator import Cascade
    bleed, mask, x = models
    eager = {T: tuple(t.clone() for t in Cascade(bleed, mask, temperature=T).predict(x)) for T in (2.0, 0.5)}
    c = Cascade(bleed, mask, temperature=2.0)
    c.capture_predict_graph(x)
    g = c._pgraph
    c.predict_inputs().copy_(x)
    out = c.predict(c.predict_inputs())
    assert out.probs.data_ptr() == c._pprobs.probs.data_ptr()
    for a, b in zip(out, eager[2.0]):
        assert _same(a, b)                                                       # the captured graph equals the eager run bit for bit
    c.set_temperature(0.5)
    out = c.predict(c.predict_inputs())
    assert c._pgraph is g and c.temperature == 0.5
    for a, b in zip(out, eager[0.5]):
        assert _same(a, b)                                                       # the replay follows the device float
    # a graph captured before any temperature holds no launch for it: the first set_temperature drops that capture
    p = Cascade(bleed, mask)
    p.capture_predict_graph(x)
    p.set_temperature(0.5)
    assert p._pgraph is None
    for a, b in zip(p.predict(x), eager[0.5]):
        assert _same(a, b)


def test_cascade_temperature_of_an_ensemble_scales_the_mean(models):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.ensemble import Ensemble
    from ultrasound_modeling_amd.TBIEvaluator import Cascade, EnsembleCascadeOutput
    bleed, mask, x = models
    plain = tuple(t.clone() for t in Cascade(Ensemble(bleed, flip=True), mask).predict(x))
    c = Cascade(Ensemble(bleed, flip=True), mask, temperature=1.5)
    out = tuple(t.clone() for t in c.predict(x))
    assert isinstance(c.predict(x), EnsembleCascadeOutput)
    scaled = ops.apply_temperature(plain[0], _beta(1.5))
    pm, bp = ops.cascade_maps(scaled)
    assert _same(out[0], scaled) and _same(out[2], pm) and _same(out[3], bp) and torch.equal(out[1], plain[1])
    for i in (4, 5, 6):                                                          # entropy, mutual_info, image_scores: the members', un-scaled
        assert _same(out[i], plain[i])
    c.capture_predict_graph(x)
    c.predict_inputs().copy_(x)
    for a, b in zip(c.predict(c.predict_inputs()), out):
        assert _same(a, b)


# ------------------------------------------------------------------------------------------------ the drivers
class _Recorder:
    def __init__(self, net):
        self.net, self.seen = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def step(self, x, y, **kw):
        out = self.net.step(x, y, **kw)
        self.seen.append((torch.as_tensor(y).float().cpu().numpy().copy(), out[-1].float().cpu().numpy().copy()))
        return out


def test_mainnumpy_process_prints_one_sweep_line(monkeypatch):
    import contextlib
    import io
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.Dataset_2 import Dataset
    from ultrasound_modeling_amd.MainNumpy import Process
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    rng = np.random.default_rng(1)
    raw = np.zeros((6, 1, 64, 64, 12), dtype=np.float64)            # label, 10 displacement channels, bMode (Dataset_2.py:33-43)
    raw[..., 1:11] = np.clip(rng.standard_normal((6, 1, 64, 64, 10)) * 0.3, -1, 1)
    raw[..., 0] = np.kron(rng.choice([0.0, 1.0, 2.0], size=(6, 1, 8, 8), p=[0.6, 0.2, 0.2]), np.ones((8, 8)))
    ds = Dataset(train_data=raw, val_data=raw[:3], num_classes=3)
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=10, learning_rate=1e-3)
    rec = _Recorder(net)
    proc = Process(batch_size=2, num_classes=3, sweep={"bins": 256, "cls": -1})
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        proc.test(rec, ds, epoch=1)
    lines = buf.getvalue().splitlines()
    y = np.concatenate([t[0] for t in rec.seen])
    p = np.concatenate([t[1] for t in rec.seen])
    want = R.sweep_from_counts(R.sweep_counts(p, y, 256, 2))
    h = proc.history[-1]
    assert h["auc"] == want["auc"] and h["average_precision"] == want["average_precision"] and 0 < h["auc"] < 1
    assert h["best_dice"] == want["best_dice"][2] and h["best_dice_threshold"] == want["best_dice"][1]
    sw = [l for l in lines if l.startswith("sweep")]
    assert len(sw) == 1 and lines.index(sw[0]) == len(lines) - 1 and "AUC = {:.5f}".format(want["auc"]) in sw[0]
    assert not bool(proc.sweep.counts.any())                         # reset for the next epoch

    # without sweep=: the parent's lines and keys, and no sweep launch
    def boom(*a, **k):
        raise AssertionError("score_sweep launched without sweep=")
    monkeypatch.setattr(ops, "score_sweep", boom)
    ds.reset_idx()
    plain = Process(batch_size=2, num_classes=3)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        plain.test(net, ds, epoch=1)
    what = lambda ls: [l.split(" = ")[0] for l in ls]
    assert what(buf.getvalue().splitlines()) == what(lines[:-1]) == ["", "Test...", "loss", "IoU", "f1", "precision", "recall"]
    assert set(plain.history[-1]) == set(h) - {"auc", "average_precision", "best_dice", "best_dice_threshold"}


def test_main_fits_a_temperature_sweeps_and_hands_the_threshold_on(tmp_path, monkeypatch, capsys):
    """``main --fit-temperature --roc-csv --threshold best-dice --lesion-csv`` with the checkpoints, the geometry and the figures stubbed out:
    the rows are ``sweep_scores``' of the calibrated probabilities, and the lesion scores use the sweep's threshold."""
    import csv
    from ultrasound_modeling_amd import TBIEvaluator as E
    bleed, mask = _arch_b(3, cin=10, seed=3), _arch_b(2, cin=10, seed=4)
    rng = np.random.default_rng(61)
    data = rng.standard_normal((3, 1, 64, 64, 12))
    data[..., 0] = 0
    names = np.array(["a", "b", "c"])
    # labels drawn from the model's own probabilities squared: the fit has an interior minimiser (beta about 2) whatever the random model says
    _, _, p0 = E._polar_run(data, E.Cascade(bleed, mask), names, 2, uncertainty=False, keep_probs=True)
    sharp = p0.astype(np.float64) ** 2
    sharp /= sharp.sum(-1, keepdims=True)
    data[..., 0] = (rng.random((3, 64, 64, 1)) > sharp.cumsum(-1)[..., :2]).sum(-1).reshape(3, 1, 64, 64)
    np.save(tmp_path / "data.npy", data)
    np.save(tmp_path / "paths.npy", names)
    made = []

    def from_checkpoints(cls, *a, **k):
        made.append(E.Cascade(bleed, mask))
        return made[-1]
    monkeypatch.setattr(E.Cascade, "from_checkpoints", classmethod(from_checkpoints))
    monkeypatch.setattr(E.ConeGeometry, "from_dir", classmethod(lambda cls, *a, **k: None))
    monkeypatch.setattr(E, "Display", lambda *a, **k: [])
    seen = {}
    real = E.write_lesion_csv
    monkeypatch.setattr(E, "write_lesion_csv", lambda path, result, *a, **k: (seen.update(k), real(path, result, *a, **k))[1])
    roc, les = tmp_path / "roc.csv", tmp_path / "les.csv"
    E.main([str(tmp_path / "data.npy"), str(tmp_path / "paths.npy"), str(tmp_path), str(tmp_path / "out"), "--bleed", "none.pt", "--batch", "2",
            "--fit-temperature", "--roc-csv", str(roc), "--sweep-bins", "64", "--threshold", "best-dice", "--lesion-csv", str(les)])
    out = capsys.readouterr().out
    assert "fitted temperature T = " in out and "wrote 65 operating points" in out and "--threshold best-dice: " in out and "sweep: AUC" in out
    T = made[0].temperature
    assert T is not None and 1 / 8 < T < 8
    _, _, probs = E._polar_run(data, E.Cascade(bleed, mask), names, 2, uncertainty=False, keep_probs=True)
    fit = E.fit_cascade_temperature(probs, data.reshape(3, 64, 64, 12)[..., 0], device=DEV)
    assert fit["temperature"] == T and fit["nll"] <= fit["nll_at_1"]
    _, _, scaled = E._polar_run(data, E.Cascade(bleed, mask, temperature=T), names, 2, uncertainty=False, keep_probs=True)
    want = E.sweep_scores(scaled, data.reshape(3, 64, 64, 12)[..., 0], bins=64, device=DEV)
    rows = list(csv.reader(open(roc)))
    assert len(rows) == 1 + 65 + 1 and rows[-1][0] == "total" and int(rows[-1][10]) == 3 * 64 * 64
    assert [int(r[2]) for r in rows[1:-1]] == want["tp"].tolist() and float(rows[-1][11]) == want["auc"]
    assert seen["threshold"] == want["best_dice"][1] == float(rows[-1][14])
