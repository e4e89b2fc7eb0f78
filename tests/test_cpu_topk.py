"""The top-k (hard-pixel) cross-entropy (usseg.h UssegTopkLoss) and the exact selection's C ABI without a GPU: the fp64 restatement
(tests/topk_restatement.py) against known answers, the oracle's CCE and finite differences; the Python surface's refusals; the header's
contract; the entry points' argument checks (which run before any launch, so they run here)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import overlap_restatement as R
import topk_restatement as T
import usseg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the restatement
def test_five_losses_two_selected_by_hand():
    """l = (0.5, 2, 0.25, 3, 1), k = 2: t = 2, one key above it, one equal, r = 1: the pixels with 3 and 2 carry weight 1, the loss is their mean."""
    l = np.array([0.5, 2.0, 0.25, 3.0, 1.0])
    t, ngt, neq = T.select(_bits(l), 2)
    assert (t, ngt, neq) == (int(_bits([2.0])[0]), 1, 1)
    assert T.weights(_bits(l), 2).tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
    cfg = T.config(fraction=0.4)
    assert T.k_of(0.4, 5) == 2
    assert T.loss(l, 5, cfg) == pytest.approx(5 / 2 * (3.0 + 2.0))                       # inv_global_batch 1: the SUM convention, times n/k
    assert T.loss(l, 5, cfg, inv_global_batch=1 / 5) == pytest.approx(2.5)             # the mean of exactly k values


def test_a_tie_straddling_the_cut_shares_the_remaining_weight():
    """l = (2, 3, 2, 0.5, 2), k = 2: t = 2, ngt = 1, neq = 3, r = 1: each of the three tied pixels gets 1/3, and the loss is still the mean of
    exactly two values (3 and one 2) - what torch.topk(l, 2).values.mean() returns."""
    l = np.array([2.0, 3.0, 2.0, 0.5, 2.0])
    assert T.select(_bits(l), 2) == (int(_bits([2.0])[0]), 1, 3)
    a = T.weights(_bits(l), 2)
    assert a.tolist() == [1 / 3, 1.0, 1 / 3, 0.0, 1 / 3] and a.sum() == pytest.approx(2.0)
    want = torch.topk(torch.tensor(l), 2).values.mean().item()
    assert T.loss(l, 5, T.config(fraction=0.4), inv_global_batch=1 / 5) == pytest.approx(want) and want == 2.5
    # the k that lands exactly on the last element of the run of ties: every tied pixel is selected whole
    assert T.weights(_bits(l), 4).tolist() == [1.0, 1.0, 1.0, 0.0, 1.0]


def test_a_nan_sorts_above_every_finite_value_and_makes_the_loss_nan():
    l = np.array([1.0, np.nan, np.inf, 0.5], dtype=np.float32)
    k = T.keys_of(l)
    assert k[1] > k[2] > k[0] > k[3]
    assert T.weights(k, 1).tolist() == [0.0, 1.0, 0.0, 0.0]
    assert np.isnan(T.loss(l.astype(np.float64), 4, T.config(fraction=0.25)))


@pytest.mark.parametrize("C_", [2, 3, 4])
def test_fraction_one_is_the_oracles_cce_loss_and_gradient(C_):
    logits, y = R.inputs(C_, 2, 9, 7)
    p = torch.softmax(logits, -1)
    l = T.pixel_loss(p.numpy(), y.numpy())
    assert np.abs(l - O.cce_label_smoothing(y, p).reshape(-1).numpy()).max() <= 1e-12
    cfg = T.config(fraction=1.0)
    want = O.compute_loss(y, p, 4).item()
    assert T.loss(l, 63, cfg, inv_global_batch=0.25) == pytest.approx(want, rel=1e-13)
    assert T.loss(l, 63, dict(cfg, scope="image"), inv_global_batch=0.25) == pytest.approx(want, rel=1e-13)
    a, k, n = T.all_weights(l.astype(np.float32), 63, cfg)
    assert (a == 1.0).all() and k == n == 126
    G, _, _ = T.dlogits_terms(p.numpy(), y.numpy(), a, k, n, cfg, 0.25)
    pc = p.clone().requires_grad_(True)
    O.compute_loss(y, pc, 4).backward()
    assert np.abs(G - pc.grad.reshape(-1, C_).numpy()).max() <= 1e-12


def test_the_count_rule():
    f = np.float32(0.1)                               # 0.100000001490116...: f*n lies just ABOVE an integer at n = 10^k
    assert float(f) > 0.1 and T.k_of(f, 10) == 1 and T.k_of(f, 1000) == 100 and T.k_of(f, 10 ** 8) == 10 ** 7
    g = np.float32(0.3)                               # 0.300000011920929
    h = np.nextafter(g, np.float32(0))                # 0.29999998211860657: f*n just BELOW the integer
    assert T.k_of(g, 10) == 3 and T.k_of(h, 10) == 2 and T.k_of(g, 20480) == 6144 and T.k_of(h, 20480) == 6143
    assert T.k_of(1.0, 7) == 7 and T.k_of(np.float32(1e-9), 7) == 1 and T.k_of(0.5, 1) == 1          # clamped to n and to 1
    assert T.k_of(0.25, 1 << 29) == 1 << 27
    # the product is exact in fp64: a 24-bit fraction times a 30-bit count
    f = np.float32(0.7654321)
    n = (1 << 29) - 3
    from fractions import Fraction
    assert T.k_of(f, n) == int(Fraction(float(f)) * n)


def test_finite_differences_on_a_stable_selection():
    """k-th and (k+1)-th largest l at least 1e-3 relative apart: a RELATIVE step of 1e-6 in a probability moves l by at most 2e-6
    (|d l / d p_c| <= 1/p_c + 1/sum p), far less than the gap, so no pixel crosses the cut, the loss is smooth on the step and its central
    difference is the stated gradient."""
    C_, B, H, W = 3, 1, 9, 7
    logits, y = R.inputs(C_, B, H, W)
    p = torch.softmax(logits.float(), -1).double().numpy().reshape(-1, C_)
    yn = y.numpy().reshape(-1, C_)
    cfg = T.config(fraction=0.25, tk_weight=0.7)
    l = T.pixel_loss(p, yn)
    a, k, n = T.all_weights(l.astype(np.float32), H * W, cfg)
    s = np.sort(l)[::-1]
    assert k == 15 and n == 63 and (s[k - 1] - s[k]) >= 1e-3 * s[k - 1], (s[k - 1], s[k])
    assert s[k - 1] - s[k] >= 100 * 2e-6
    G, _, _ = T.dlogits_terms(p, yn, a, k, n, cfg, 0.5)
    checked = 0
    for m in list(np.nonzero(a == 1.0)[0][:8]) + list(np.nonzero(a == 0.0)[0][:4]):
        for c in range(C_):
            h = 1e-6 * p[m, c]

            def at(delta):
                q = p.copy()
                q[m, c] += delta
                return T.loss(T.pixel_loss(q, yn), H * W, cfg, 0.5)
            fd = (at(h) - at(-h)) / (2 * h)
            assert abs(fd - G[m, c]) <= 1e-6 * max(abs(G[m, c]), 1e-3), (m, c, fd, G[m, c])
            checked += 1
    assert checked == 36 and not G[a == 0.0].any()


def test_image_scope_is_the_sum_of_the_per_image_calls():
    C_, B, H, W = 3, 3, 9, 7
    logits, y = R.inputs(C_, B, H, W)
    p = torch.softmax(logits, -1).numpy()
    cfg = T.config(fraction=0.2, scope="image")
    l = T.pixel_loss(p, y.numpy())
    whole = T.loss(l, H * W, cfg, 1 / 3)
    parts = [T.loss(T.pixel_loss(p[b], y.numpy()[b]), H * W, dict(cfg, scope="batch"), 1 / 3) for b in range(B)]
    assert whole == pytest.approx(sum(parts), rel=1e-14)
    assert whole != pytest.approx(T.loss(l, H * W, dict(cfg, scope="batch"), 1 / 3), rel=1e-6)       # (the batch selection is another loss)


def test_the_dice_topk_sum_rule():
    """loss("dice_topk") = L_tk + the Dice loss with ce_weight 0, as ``topk_config`` resolves the two halves."""
    from ultrasound_modeling_amd.VisionTransformer import overlap_config, topk_config
    tk, f, ov = topk_config("dice_topk", 3, dict(fraction=0.25, tk_weight=0.5), overlap=dict(smooth=2.0))
    ref = overlap_config("dice", 3, dict(smooth=2.0))
    assert (tk.tk_weight, tk.scope, f) == (0.5, 0, 0.25)
    assert bytes(ov) == bytes(ref) and ov.ce_weight == 0.0 and ov.alpha == ov.beta == 0.5 and ov.smooth == 2.0
    assert topk_config("topk", 3, None)[2] is None


def test_the_gpu_tests_inputs_stay_away_from_the_cce_clip_edges():
    """tests/test_gpu_topk.py runs on overlap_restatement.inputs, whose normalised probabilities lie nowhere within 2^-20 relative of a clip
    constant: no pixel has to be left out of a per-element comparison."""
    for C_ in (2, 3, 4):
        for B, H, W in ((2, 256, 80), (1, 64, 47), (1, 64, 46), (1, 9, 7), (1, 1, 1), (3, 10, 6)):
            logits, _ = R.inputs(C_, B, H, W)
            q = torch.softmax(logits, -1)
            rel = 2.0 ** -20
            assert int((((q - R.LO).abs() <= rel * R.LO) | ((q - R.HI).abs() <= rel * R.HI)).sum()) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_refuses_bad_topk_losses():
    from ultrasound_modeling_amd import ops
    for kw in (dict(tk_weight=-1.0), dict(tk_weight=float("nan")), dict(tk_weight=float("inf")), dict(scope="pixel"), dict(scope=0)):
        with pytest.raises(ValueError):
            ops.topk_loss(**kw)
    for f in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.topk_fraction_value(f)
    assert ops.topk_fraction_value(1) == 1.0 and ops.topk_fraction_value(1e-9) == 1e-9
    tk = ops.topk_loss(0.25, "image")
    assert (tk.tk_weight, tk.scope) == (0.25, 1)
    assert ops.TOPK_KEYS == ("fraction", "scope", "tk_weight") and ops.TOPK_SCOPES == ("batch", "image")


def test_the_new_names_are_accepted_where_they_used_to_raise():
    from ultrasound_modeling_amd import MainParallel
    from ultrasound_modeling_amd.VisionTransformer import TOPK_LOSSES, VisionTransformer, topk_config
    assert TOPK_LOSSES == ("topk", "dice_topk")
    f = lambda r: (r[0].tk_weight, r[0].scope, r[1])
    assert f(topk_config("topk", 3, None)) == (1.0, 0, 0.1) and f(topk_config("dice_topk", 3, {})) == (1.0, 0, 0.1)
    assert f(topk_config("topk", 2, dict(fraction=0.5, scope="image", tk_weight=2))) == (2.0, 1, 0.5)
    for loss in TOPK_LOSSES:
        try:                                # past every ValueError: the constructor goes on to the device (and needs one)
            net = VisionTransformer(2, (64, 64), in_channels=1, loss=loss)
            assert net.topk_loss is not None and net.loss_name == loss
        except RuntimeError as e:
            assert "HIP device" in str(e)
    src = inspect.getsource(MainParallel._cli)
    assert '("topk", "dice_topk")' in src and "--topk-fraction" in src and "--topk-scope" in src


def test_topk_config_refusals():
    from ultrasound_modeling_amd.VisionTransformer import topk_config
    for loss, cfg, kw in (("topk", dict(bogus=1), {}), ("topk", dict(fraction=0.0), {}), ("topk", dict(fraction=1.5), {}),
                          ("topk", dict(fraction=float("nan")), {}), ("topk", dict(scope="pixel"), {}), ("topk", dict(tk_weight=-1.0), {}),
                          ("topk", [0.1], {}), ("cce", {}, {}), ("dice", dict(fraction=0.2), {}), ("lovasz", None, {}),
                          ("topk", None, dict(class_factor=[1, 1, 1])), ("dice_topk", None, dict(focal_gamma=2.0)), ("topk", None, dict(boundary={})),
                          ("dice_topk", None, dict(boundary=dict(weight=0.1))), ("topk", None, dict(lovasz={})), ("topk", None, dict(overlap={})),
                          ("topk", None, dict(overlap=dict(smooth=2.0))), ("dice_topk", None, dict(overlap=dict(ce_weight=1.0))),
                          ("dice_topk", None, dict(overlap=dict(alpha=0.3))), ("dice_topk", None, dict(overlap=dict(bogus=1)))):
        with pytest.raises(ValueError):
            topk_config(loss, 3, cfg, **kw)


def test_constructor_refusals_come_before_any_device_work():
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for kw in (dict(loss="topk", topk=dict(bogus=1)), dict(loss="topk", topk=dict(fraction=0.0)), dict(loss="topk", topk=dict(fraction=2.0)),
               dict(loss="dice_topk", topk=dict(scope="pixel")), dict(loss="cce", topk={}), dict(loss="dice", overlap={}, topk={}),
               dict(loss="lovasz", topk=dict(fraction=0.2)), dict(loss="topk", class_factor=[1, 1, 1]), dict(loss="dice_topk", focal_gamma=2.0),
               dict(loss="topk", boundary={}), dict(loss="dice_topk", boundary=dict(weight=0.1)), dict(loss="topk", lovasz={}),
               dict(loss="topk", overlap={}), dict(loss="topk", smooth=2.0), dict(loss="dice_topk", overlap=dict(ce_weight=1.0)),
               dict(loss="dice_topk", ce_weight=0.5), dict(loss="dice_topk", num_classes=2, overlap=dict(class_weight=[1, 1, 1]))):
        with pytest.raises(ValueError):
            VisionTransformer(2, (64, 64), in_channels=1, **kw)
        with pytest.raises(ValueError):
            TransUNet((64, 64), batch_size=2, in_channels=1, **kw)


def test_drivers_take_the_topk_settings_and_refuse_contradictions():
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main, VisionTransformer.__init__, TBI_TransUNet.VisionTransformer.__init__):
        par = inspect.signature(fn).parameters
        assert par["loss"].default == "cce" and par["topk"].default is None and par["topk"].kind is inspect.Parameter.KEYWORD_ONLY, fn
    for argv in (["a.npy", "b.npy", "--topk-fraction", "0.2"], ["a.npy", "b.npy", "--loss", "dice", "--topk-scope", "image"],
                 ["a.npy", "b.npy", "--loss", "topk", "--topk-fraction", "0"], ["a.npy", "b.npy", "--loss", "topk", "--topk-fraction", "1.5"],
                 ["a.npy", "b.npy", "--loss", "topk", "--topk-scope", "pixel"], ["a.npy", "b.npy", "--loss", "topk", "--boundary-weight", "0.1"]):
        with pytest.raises(SystemExit):
            MainParallel._cli(argv)


def test_the_dice_line_appears_for_a_topk_model():
    import types
    from ultrasound_modeling_amd import metrics
    seg = types.SimpleNamespace(dice=lambda: [1.0])
    assert metrics.dice_line(types.SimpleNamespace(overlap_loss=None, lovasz_loss=None, topk_loss=object()), seg) == [1.0]
    assert metrics.dice_line(types.SimpleNamespace(overlap_loss=None, lovasz_loss=None, topk_loss=None), seg) is None


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _desc(L, C_=3, M=32, HW=16, lddl=8, quad_w=0, eps=1e-7, ls=0.1, inv=0.25):
    return L.LossDesc(M, HW, C_, C_, lddl, 0, ls, eps, inv, quad_w)


def test_struct_layout_symbols_and_the_headers_contract():
    L, lib = _lib()
    assert C.sizeof(L.TopkLoss) == 8
    assert {n: getattr(L.TopkLoss, n).offset for n, _ in L.TopkLoss._fields_} == dict(tk_weight=0, scope=4)
    names = ("usseg_topk_select_ws_bytes", "usseg_topk_select", "usseg_topk_ws_bytes", "usseg_topk_pixel_loss", "usseg_topk_loss_sums", "usseg_topk_loss_bwd")
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in names:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\(", hdr), name
    flat = " ".join(re.sub(r"(?m)^ \* ?", "", hdr).split())
    for phrase in ("k = max(1, min(n, floor((double)f * n)))", "read from DEVICE memory when the kernels run", "On the device the clamp is the whole rule",
                   "with the sign bit cleared", "a NaN sorts above every finite value","Ties are shared, not broken by index",
                   "the mean of exactly k values", "A pixel with a(m) = 0 stores exact zeros in all its slots", "ONE bf16 rounding",
                   "usseg_overlap_loss_sums runs unchanged with ce_weight = 0", "Seven kernels and one memset", "Five kernels and one memset",
                   "No workgroup waits for another", "Only integer atomics are used", "never by the data", "No host synchronisation, no allocation",
                   "usseg_overlap_loss_grid(M)", "pad channels are exactly zero", "M = 0 gives loss 0", "Every argument is checked before any launch",
                   "typedef struct UssegTopkLoss"):
        assert phrase in flat, phrase
    # the sizes the header's rule gives
    from ultrasound_modeling_amd import ops
    a = lambda b: (b + 255) // 256 * 256
    for M, HW in ((1, 1), (63, 63), (2 * 20480, 20480), (6 * 35, 35)):
        for scope in ("batch", "image"):
            S = M // HW if scope == "image" else 1
            assert ops.topk_select_ws_bytes(S) == S * 4 * 256 * 4
            assert ops.topk_ws_bytes(M, HW, scope) == a(4 * M) + a(S * 4096) + a(16 * S)
    assert ops.topk_ws_bytes(0, 16) == 0
    assert lib.usseg_topk_ws_bytes((1 << 29) + 16, 16, 0) == -1 and lib.usseg_topk_ws_bytes(33, 16, 0) == -1 and lib.usseg_topk_ws_bytes(32, 16, 2) == -1
    assert lib.usseg_topk_ws_bytes(32, 0, 0) == -1 and lib.usseg_topk_select_ws_bytes(-1) == -1 and lib.usseg_topk_select_ws_bytes((1 << 29) + 1) == -1


def test_the_select_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()
    need = lib.usseg_topk_select_ws_bytes(3)

    def call(keys=16, S=3, n=5000, frac=None, k=500, sel=32, ws=128, ws_bytes=need):
        return lib.usseg_topk_select(keys, S, n, frac, k, sel, ws, ws_bytes, None)
    assert call(ws_bytes=need - 1) == -1 and f"topk_select: the workspace holds {need - 1} bytes, {need} needed" in err()
    for kw in (dict(keys=None), dict(sel=None), dict(ws=None)):
        assert call(**kw) == -1 and "topk_select: null pointer" in err(), kw
    for kw in (dict(keys=18), dict(sel=36), dict(ws=132), dict(frac=18, k=0)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(frac=64, k=5) == -1 and "not both and not neither" in err() and call(k=0) == -1 and "not both and not neither" in err()
    assert call(k=5001) == -1 and "1 <= k <= n" in err() and call(k=-1) == -1
    assert call(S=-1) == -1 and "segments" in err()
    assert call(n=0) == -1 and "2^29" in err() and call(n=(1 << 29) + 1) == -1
    assert call(S=0) == 0                                            # nothing to do, nothing launched


@pytest.mark.parametrize("entry", ["topk_pixel_loss", "topk_loss_sums", "topk_loss_bwd"])
def test_the_loss_entry_points_refuse_bad_arguments_before_any_launch(entry):
    """Non-null dummy pointers (aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()
    ACC = 8224

    def call(d=None, tk=None, frac=16, probs=16, y_true=16, ws=16, ws_bytes=1 << 30, ov=None, acc=32, acc_floats=ACC, dl=16):
        d = C.byref(d) if d is not None else None
        tk = L.TopkLoss(1.0, 0) if tk is None else tk
        if entry == "topk_pixel_loss":
            return lib.usseg_topk_pixel_loss(d, tk, frac, probs, y_true, ws, ws_bytes, None)
        if entry == "topk_loss_sums":
            return lib.usseg_topk_loss_sums(d, tk, ws, ws_bytes, ov, acc, acc_floats, None)
        return lib.usseg_topk_loss_bwd(d, tk, probs, y_true, ws, ws_bytes, acc, acc_floats, ov, dl, None)

    assert call(d=None) == -1 and f"{entry}: null descriptor" in err()
    for bad_c in (0, 5):
        assert call(d=_desc(L, C_=bad_c)) == -1 and f"{entry}: 1 <= C <= 4" in err()
    for d in (_desc(L, M=33), _desc(L, HW=0), _desc(L, M=-16)):
        assert call(d=d) == -1 and "M must be a non-negative multiple of HW" in err()
    assert call(d=_desc(L, M=(1 << 29) + 16)) == -1 and "more than 2^29 pixels" in err()
    for w in (-1.0, float("nan"), float("inf")):
        assert call(d=_desc(L), tk=L.TopkLoss(w, 0)) == -1 and "tk_weight must be finite and >= 0" in err(), w
    for scope in (-1, 2):
        assert call(d=_desc(L), tk=L.TopkLoss(1.0, scope)) == -1 and "scope must be 0 (batch) or 1 (image)" in err()
    assert call(d=_desc(L, inv=-1.0)) == -1 and "inv_global_batch" in err()
    assert call(d=_desc(L, ls=1.0)) == -1 and "label_smoothing" in err()
    assert call(d=_desc(L, eps=0.0)) == -1 and "clip_eps" in err()
    for scope in (0, 1):
        need = lib.usseg_topk_ws_bytes(32, 16, scope)
        assert call(d=_desc(L), tk=L.TopkLoss(1.0, scope), ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    assert call(d=_desc(L), ws=None) == -1 and call(d=_desc(L), ws=20) == -1 and "workspace" in err()
    if entry != "topk_loss_sums":
        for kw in (dict(probs=None), dict(y_true=None)):
            assert call(d=_desc(L), **kw) == -1 and f"{entry}: null pointer" in err(), kw
        for kw in (dict(probs=20), dict(y_true=24)):
            assert call(d=_desc(L), **kw) == -1 and "16-byte aligned" in err(), kw
    if entry == "topk_pixel_loss":
        assert call(d=_desc(L), frac=None) == -1 and "fraction" in err() and call(d=_desc(L), frac=18) == -1
        assert call(d=_desc(L, M=0)) == 0                     # nothing to do, nothing launched
    elif entry == "topk_loss_sums":
        assert call(d=_desc(L, M=2 * 256 * 80, HW=256 * 80), acc_floats=32 + 16 * 39) == -1 and "a grid of 40 workgroups needs 672 accumulator floats" in err()
        assert call(d=_desc(L), acc=None) == -1 and call(d=_desc(L), ov=32) == -1 and "overlap_acc" in err()
    else:
        assert call(d=_desc(L), acc_floats=31) == -1 and "header floats" in err()
        assert call(d=_desc(L), dl=None) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
        assert call(d=_desc(L, lddl=16)) == -1 and "dlogits stride" in err()
        assert call(d=_desc(L, lddl=16, quad_w=3)) == -1 and "quad layout" in err()
        assert call(d=_desc(L, M=0)) == 0                     # nothing to do, nothing launched
