"""The Lovasz-softmax loss (usseg.h UssegLovaszLoss) and the radix sort's C ABI without a GPU: the fp64 restatement (tests/lovasz_restatement.py)
against the paper's listing, known answers, finite differences; the Python surface's refusals; the header's contract; the entry points'
argument checks (which run before any launch, so they run here)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lovasz_restatement as V
import overlap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p32(logits):
    return torch.softmax(logits.float(), -1).contiguous()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,frac", [(1, 0.5), (7, 0.3), (63, 0.0), (63, 1.0), (4096, 0.01), (40960, 0.01), (40960, 0.5)])
def test_the_closed_form_is_the_papers_cumsum_form(n, frac):
    """g from the exact integers equals the first differences of the Jaccard losses of the sorted prefixes.  The difference form carries the
    cancellation error of two numbers near 1 (about 2^-53 absolute each), the closed form one division: the two agree to 4 * 2^-53 ABSOLUTE
    per element, and both sum to 1 (or to the last Jaccard loss, 1 - 0 = 1)."""
    rng = np.random.default_rng(n + int(100 * frac))
    fg = rng.random(n) < frac
    a, b = V.grad_closed(fg), V.grad_paper(fg)
    assert np.abs(a - b).max() <= 4 * 2.0 ** -53
    assert (a >= 0).all() and abs(a.sum() - 1.0) <= n * 2.0 ** -53
    if not fg.any():
        assert a[0] == 1.0 and not a[1:].any()


def test_the_order_is_key_descending_with_ties_by_index():
    e = np.array([0.25, 1.0, 0.25, 0.0, 7.0, np.nan, -0.25, 0.5], dtype=np.float32)
    k = V.keys(e)
    assert k[1] == k[4] == k[5] == V.ONE_BITS and k[0] == k[2] == k[6]          # clamped at 1.0 (NaN and 7 included); |e| decides
    assert V.order(k).tolist() == [1, 4, 5, 7, 0, 2, 6, 3]
    assert int(k.max()) < 1 << V.KEY_BITS


@pytest.mark.parametrize("C_", [2, 3, 4])
def test_hard_predictions_give_one_minus_the_iou(C_):
    """p in {0, 1}: every error is 0 or 1, the errors of size 1 come first, and the sum of g over them telescopes to the Jaccard loss."""
    gen = torch.Generator().manual_seed(5 + C_)
    lab = torch.randint(0, C_, (2, 16, 12), generator=gen)
    pred = torch.where(torch.rand(2, 16, 12, generator=gen) < 0.7, lab, torch.randint(0, C_, (2, 16, 12), generator=gen))
    y = torch.nn.functional.one_hot(lab, C_).double()
    p = torch.nn.functional.one_hot(pred, C_).double()
    Lc, _, counts = V.per_class(p, y, V.config(C=C_))
    for c in range(C_):
        inter = ((pred == c) & (lab == c)).sum().item()
        union = ((pred == c) | (lab == c)).sum().item()
        assert counts[c] == (lab == c).sum().item()
        assert abs(Lc[c].item() - (1.0 - inter / union)) <= 1e-12


def test_two_pixels_by_hand():
    """One class column, two pixels: foreground with p = 0.6 (e = 0.4), background with p = 0.7 (e = 0.7).  Order: the background pixel first.
    Y = 1.  Rank 0 (background): F = 0, I = 1, U = 2, g = 1/(2*1) = 0.5.  Rank 1 (foreground): F = 1, U = 1 + 2 - 1 = 2, g = 0.5."""
    p = torch.tensor([[0.6, 0.4], [0.7, 0.3]], dtype=torch.float32).double()
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    Lc, g, counts = V.per_class(p, y, V.config(C=2))
    assert counts.tolist() == [1, 1] and np.allclose(g[:, 0], [0.5, 0.5])
    assert abs(Lc[0].item() - (0.5 * float(np.float32(1) - np.float32(0.6)) + 0.5 * float(np.float32(0.7)))) <= 1e-7


@pytest.mark.parametrize("loss", ["lovasz", "lovasz_ce"])
@pytest.mark.parametrize("classes", ["present", "all"])
def test_finite_differences_at_pixels_with_a_unique_key(loss, classes):
    """The loss is linear in p on the piece its order defines: at a pixel whose error is at least 1e-4 away from every other error of its class a
    central difference with h = 1e-6 stays on the piece and equals the stated gradient k_c * (fg ? -1 : +1) * g (+ the CCE term)."""
    C_, B, H, W = 3, 1, 9, 7
    logits, y = V.inputs("gauss", C_, B, H, W)
    cfg = V.config(loss, C_, w=[0.2, 0.3, 0.5], lv_weight=0.7, classes=classes)
    p32 = _p32(logits)
    want = V.restate_at(p32, y, cfg, 0.25, 0.5)
    p = p32.double()
    fg = V.foreground(y.numpy().reshape(-1, C_))
    e = V.errors32(p32.numpy().reshape(-1, C_), fg).astype(np.float64)
    sign = np.where(fg, -1.0, 1.0)
    stated = want["k"] * sign * want["g"].reshape(-1, C_)
    h, checked = 1e-6, 0
    for c in range(C_):
        d = np.abs(e[:, c][:, None] - e[:, c][None, :]) + np.eye(e.shape[0])
        for m in np.nonzero(d.min(1) >= 1e-4)[0][:12]:
            def at(delta):
                q = p.clone().reshape(-1, C_)
                q[m, c] += delta
                cfg0 = dict(cfg, ce_weight=0.0)
                return V.loss(q.reshape(p.shape), y, cfg0, 0.25, 0.5).item()
            fd = (at(h) - at(-h)) / (2 * h)
            assert abs(fd - stated[m, c]) <= 1e-7 * max(abs(stated[m, c]), 1e-3), (c, m, fd, stated[m, c])
            checked += 1
    assert checked >= 20
    G = want["G"].reshape(-1, C_).numpy()
    if cfg["ce_weight"] == 0.0:
        assert np.abs(G - stated).max() <= 1e-15
    else:
        pc = p.clone().requires_grad_(True)
        (cfg["ce_weight"] * 0.25 * R.cce_per_pixel(pc, y).sum()).backward()
        assert np.abs(G - stated - pc.grad.reshape(-1, C_).numpy()).max() <= 1e-12


@pytest.mark.parametrize("kind", ["absent", "full"])
def test_absent_and_all_foreground_classes_under_both_settings(kind):
    C_, B, H, W = 3, 1, 9, 7
    logits, y = V.inputs(kind, C_, B, H, W)
    p32 = _p32(logits)
    pres = V.restate_at(p32, y, V.config(C=C_), 1.0, 1.0)
    full = V.restate_at(p32, y, V.config(C=C_, classes="all"), 1.0, 1.0)
    counts = pres["counts"].tolist()
    absent = [c for c in range(C_) if counts[c] == 0]
    assert absent == ([2] if kind == "absent" else [1, 2]) and (kind != "full" or counts[0] == B * H * W)
    for c in absent:      # Y = 0: g is 1 at the largest error and 0 elsewhere, so L_c is the largest probability of the class
        g = pres["g"].reshape(-1, C_)[:, c]
        assert g.sum() == 1.0 and g.max() == 1.0 and abs(pres["L"][c].item() - p32[..., c].max().item()) <= 1e-12
        assert pres["k"][c] == 0.0 and not pres["G"][..., c].any()            # "present": no weight, no gradient
        assert full["k"][c] == pytest.approx(1.0 / C_) and full["G"][..., c].abs().sum().item() == pytest.approx(1.0 / C_)
    n = C_ - len(absent)
    assert pres["loss"] == pytest.approx(sum(pres["L"][c].item() for c in range(C_) if c not in absent) / n)
    assert full["loss"] == pytest.approx(pres["L"].sum().item() / C_)
    if kind == "full":    # every pixel foreground: U = Y at every rank, g = 1/M, L_0 = the mean error
        assert np.allclose(pres["g"].reshape(-1, C_)[:, 0], 1.0 / (B * H * W), rtol=1e-15)


def test_no_class_present_gives_a_zero_loss_and_gradient():
    logits, y = V.inputs("gauss", 3, 1, 9, 7)
    r = V.restate_at(_p32(logits), torch.zeros_like(y), V.config(C=3), 1.0, 1.0)
    assert r["loss"] == 0.0 and not r["G"].any() and not r["k"].any()


def test_the_default_inputs_have_ties_and_the_generators_many_more():
    for C_ in (2, 3, 4):
        logits, y = V.inputs("gauss", C_, 2, 256, 80)
        base = V.ties(_p32(logits).numpy(), y.numpy())
        assert min(base) >= 8, base                       # the tie-break is exercised by the plain inputs already
        for kind in ("quantised", "saturated"):
            logits, y = V.inputs(kind, C_, 2, 256, 80)
            t = V.ties(_p32(logits).numpy(), y.numpy())
            assert min(t) >= 100 * max(base) and min(t) >= 2 * 256 * 80 // 4, (kind, t, base)      # a hundred times more, a quarter of the pixels
    logits, y = V.inputs("saturated", 3, 2, 256, 80)
    p = _p32(logits)
    assert (p == 0).sum().item() > 1000 and (p == 1).sum().item() > 1000


def test_the_gpu_tests_inputs_stay_away_from_the_cce_clip_edges():
    """The lovasz_ce cases of tests/test_gpu_lovasz.py run on the gauss inputs: overlap_restatement.inputs, whose normalised probabilities lie
    nowhere within 2^-20 relative of a clip constant (tests/test_cpu_overlap_loss.py checks the same shapes; (3, 10, 6) and 64x46 here)."""
    for C_ in (2, 3, 4):
        for B, H, W in ((1, 64, 46), (3, 10, 6), (2, 256, 80), (1, 64, 47), (1, 9, 7), (1, 1, 1)):
            logits, _ = V.inputs("gauss", C_, B, H, W)
            q = torch.softmax(logits, -1)
            rel = 2.0 ** -20
            assert int((((q - R.LO).abs() <= rel * R.LO) | ((q - R.HI).abs() <= rel * R.HI)).sum()) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_refuses_bad_lovasz_losses():
    from ultrasound_modeling_amd import ops
    for kw in (dict(class_weight=[1.0] * 5), dict(class_weight=[]), dict(class_weight=[1, -1, 1]), dict(class_weight=[1, 1, float("nan")]),
               dict(class_weight=[1, 1, 1], lv_weight=-1.0), dict(class_weight=[1, 1, 1], ce_weight=float("inf")),
               dict(class_weight=[1, 1, 1], threshold=float("nan")), dict(class_weight=[1, 1, 1], classes="some"),
               dict(class_weight=[1, 1, 1], lv_weight=0.0, ce_weight=0.0)):
        with pytest.raises(ValueError):
            ops.lovasz_loss(**kw)
    ll = ops.lovasz_loss([0.2, 0.3, 0.5], 0.25, 0.75, 0.4, "all")
    assert [round(v, 6) for v in list(ll.w)[:3]] + [ll.lv_weight, ll.ce_weight, round(ll.threshold, 6), ll.all_classes] == [0.2, 0.3, 0.5, 0.25, 0.75, 0.4, 1]
    assert ops.LOVASZ_KEYS == ("classes", "class_weight", "lv_weight", "ce_weight", "threshold")


def test_lovasz_config_defaults_and_refusals():
    from ultrasound_modeling_amd.VisionTransformer import LOVASZ_LOSSES, lovasz_config
    assert LOVASZ_LOSSES == ("lovasz", "lovasz_ce")
    f = lambda ll: (list(ll.w)[:3], ll.lv_weight, ll.ce_weight, ll.threshold, ll.all_classes)
    assert f(lovasz_config("lovasz", 3, None)) == ([1.0] * 3, 1.0, 0.0, 0.5, 0)
    assert f(lovasz_config("lovasz_ce", 3, {})) == ([1.0] * 3, 1.0, 1.0, 0.5, 0)
    ll = lovasz_config("lovasz_ce", 2, dict(classes="all", class_weight=[0.25, 0.75], lv_weight=2, ce_weight=0.5, threshold=0.25))
    assert (list(ll.w)[:2], ll.lv_weight, ll.ce_weight, ll.threshold, ll.all_classes) == ([0.25, 0.75], 2.0, 0.5, 0.25, 1)
    for loss, cfg in (("lovasz", dict(ce_weight=1.0)), ("lovasz_ce", dict(ce_weight=0.0)), ("lovasz", dict(smooth=1.0)), ("lovasz", dict(alpha=0.3)),
                      ("lovasz", dict(class_weight=[0.5, 0.5])), ("lovasz", dict(classes="most")), ("lovasz", dict(lv_weight=0.0)),
                      ("lovasz", dict(lv_weight=-1.0)), ("lovasz_ce", dict(threshold=float("nan"))), ("lovasz", [1, 1, 1])):
        with pytest.raises(ValueError):
            lovasz_config(loss, 3, cfg)


def test_drivers_and_constructors_take_the_lovasz_settings():
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main, VisionTransformer.__init__, TBI_TransUNet.VisionTransformer.__init__):
        par = inspect.signature(fn).parameters
        assert par["loss"].default == "cce" and par["lovasz"].default is None and par["lovasz"].kind is inspect.Parameter.KEYWORD_ONLY, fn
    src = inspect.getsource(MainParallel._cli)
    assert '"lovasz", "lovasz_ce"' in src
    with pytest.raises(SystemExit):
        MainParallel._cli(["a.npy", "b.npy", "--loss", "lovasz", "--boundary-weight", "0.1"])


def test_constructor_refusals_come_before_any_device_work():
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for kw in (dict(loss="lovasz", lovasz=dict(ce_weight=1.0)), dict(loss="lovasz_ce", lovasz=dict(ce_weight=0.0)), dict(loss="lovasz", lovasz=dict(bogus=1)),
               dict(loss="cce", lovasz={}), dict(loss="dice", overlap={}, lovasz={}), dict(loss="lovasz", boundary={}), dict(loss="lovasz_ce", boundary=dict(weight=0.1)),
               dict(loss="lovasz", overlap={}), dict(loss="lovasz", smooth=2.0), dict(loss="lovasz", class_factor=[1, 1, 1]), dict(loss="lovasz_ce", focal_gamma=2.0),
               dict(loss="lovasz", num_classes=2, lovasz=dict(class_weight=[1, 1, 1]))):
        with pytest.raises(ValueError):
            VisionTransformer(2, (64, 64), in_channels=1, **kw)
        with pytest.raises(ValueError):
            TransUNet((64, 64), batch_size=2, in_channels=1, **kw)


def test_the_dice_line_appears_for_a_lovasz_model_and_otherwise_only_for_overlap_models():
    from ultrasound_modeling_amd import metrics
    import types
    seg = types.SimpleNamespace(dice=lambda: [1.0])
    assert metrics.dice_line(types.SimpleNamespace(overlap_loss=None, lovasz_loss=object()), seg) == [1.0]
    assert metrics.dice_line(types.SimpleNamespace(overlap_loss=object()), seg) == [1.0]
    assert metrics.dice_line(types.SimpleNamespace(overlap_loss=None, lovasz_loss=None), seg) is None
    assert metrics.dice_line(types.SimpleNamespace(), seg) is None


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _ll(L, w=(0.2, 0.3, 0.5), lv_weight=1.0, ce_weight=1.0, threshold=0.5, all_classes=0):
    w = list(w) + [0.0] * (8 - len(w))
    return L.LovaszLoss((C.c_float * 8)(*w), lv_weight, ce_weight, threshold, all_classes)


def _desc(L, C_=3, M=32, HW=16, lddl=8, quad_w=0, eps=1e-7, ls=0.1, inv=0.25):
    return L.LossDesc(M, HW, C_, C_, lddl, 0, ls, eps, inv, quad_w)


def test_struct_layout_symbols_and_the_headers_contract():
    L, lib = _lib()
    assert C.sizeof(L.LovaszLoss) == 48
    off = {n: getattr(L.LovaszLoss, n).offset for n, _ in L.LovaszLoss._fields_}
    assert off == dict(w=0, lv_weight=32, ce_weight=36, threshold=40, all_classes=44)
    for name in ("usseg_sort_pairs_u32", "usseg_sort_ws_bytes", "usseg_lovasz_ws_bytes", "usseg_lovasz_coeffs", "usseg_lovasz_loss_sums", "usseg_lovasz_loss_bwd"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    from ultrasound_modeling_amd import ops
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    assert f"#define USSEG_SORT_TILE {ops.SORT_TILE}\n" in hdr and f"#define USSEG_SORT_DIGIT_BITS {ops.SORT_DIGIT_BITS}\n" in hdr
    flat = " ".join(re.sub(r"(?m)^ \* ?", "", hdr).split())
    for phrase in ("ascending on the low key_bits bits of the key and STABLE", "Bits above key_bits are ignored for the order and kept in the output",
                   "never by the data", "No host synchronisation, no allocation", "No workgroup waits for another", "Only integer atomics are used",
                   "a NaN is not foreground", "clamped to 0x3F800000", "key descending, ties by ascending pixel index", "I / (U * (U - 1))",
                   "never as a difference of two Jaccard values", "an empty S gives L_lv = 0 and a zero gradient", "usseg_overlap_loss_grid(M)",
                   "pad channels are exactly zero", "M = 0 gives loss 0", "Every argument is checked before any launch", "typedef struct UssegLovaszLoss"):
        assert phrase in flat, phrase
    # the sizes the header's rule gives
    T = ops.SORT_TILE
    a = lambda b: (b + 255) // 256 * 256
    for S, n in ((1, 1), (3, T), (4, 3 * T + 17), (3, 16 * 256 * 80)):
        assert ops.sort_ws_bytes(S, n) == 2 * a(4 * S * n) + a(4 * S * ((n + T - 1) // T) * 256)
    assert lib.usseg_sort_ws_bytes(1, (1 << 29) + 1) == -1 and lib.usseg_sort_ws_bytes(65536, 1) == -1 and lib.usseg_lovasz_ws_bytes(16, 5) == -1
    assert ops.lovasz_ws_bytes(0, 3) == 0


def test_the_sort_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()
    need = lib.usseg_sort_ws_bytes(3, 5000)

    def call(ki=16, vi=32, S=3, n=5000, bits=32, ko=48, vo=64, ws=128, ws_bytes=need):
        return lib.usseg_sort_pairs_u32(ki, vi, S, n, bits, ko, vo, ws, ws_bytes, None)
    assert call(ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    for kw in (dict(ki=None), dict(vi=None), dict(ko=None), dict(vo=None), dict(ws=None)):
        assert call(**kw) == -1 and "sort_pairs_u32: null pointer" in err(), kw
    for kw in (dict(ki=18), dict(vo=66), dict(ws=132)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(ko=16), dict(vo=32), dict(vo=48)):
        assert call(**kw) == -1 and "must not alias" in err(), kw
    for bits in (0, 33, -1):
        assert call(bits=bits) == -1 and "1 <= key_bits <= 32" in err()
    assert call(S=-1) == -1 and "segments" in err() and call(S=65536) == -1
    assert call(n=-1) == -1 and "2^29" in err() and call(n=(1 << 29) + 1) == -1
    assert call(S=0) == 0 and call(n=0) == 0                       # nothing to do, nothing launched


@pytest.mark.parametrize("entry", ["lovasz_coeffs", "lovasz_loss_sums", "lovasz_loss_bwd"])
def test_the_loss_entry_points_refuse_bad_arguments_before_any_launch(entry):
    """Non-null dummy pointers (aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()
    ACC = 8224

    def call(d=None, ll=None, probs=16, y_true=16, g=16, counts=16, ws=16, ws_bytes=1 << 30, acc=16, acc_floats=ACC, dl=16, ov_scale=1.0):
        d = C.byref(d) if d is not None else None
        ll = _ll(L) if ll is None else ll
        if entry == "lovasz_coeffs":
            return lib.usseg_lovasz_coeffs(d, ll, probs, y_true, g, counts, ws, ws_bytes, None)
        if entry == "lovasz_loss_sums":
            return lib.usseg_lovasz_loss_sums(d, ll, ov_scale, probs, y_true, g, counts, acc, acc_floats, None)
        return lib.usseg_lovasz_loss_bwd(d, ll, probs, y_true, g, acc, acc_floats, dl, None)

    assert call(d=None) == -1 and f"{entry}: null descriptor" in err()
    for kw in (dict(probs=None), dict(y_true=None), dict(g=None)):
        assert call(d=_desc(L), **kw) == -1 and f"{entry}: null pointer" in err(), kw
    for bad_c in (0, 5):
        assert call(d=_desc(L, C_=bad_c)) == -1 and f"{entry}: 1 <= C <= 4" in err()
    for d in (_desc(L, M=33), _desc(L, HW=0), _desc(L, M=-16)):
        assert call(d=d) == -1 and "M must be a non-negative multiple of HW" in err()
    assert call(d=_desc(L, M=(1 << 29) + 16)) == -1 and "more than 2^29 pixels" in err()
    for kw in (dict(probs=20), dict(y_true=24), dict(g=20)):
        assert call(d=_desc(L), **kw) == -1 and "16-byte aligned" in err(), kw
    for kw in (dict(lv_weight=-1.0), dict(ce_weight=float("nan")), dict(lv_weight=float("inf"))):
        assert call(d=_desc(L), ll=_ll(L, **kw)) == -1 and "lv_weight and ce_weight must be finite and >= 0" in err(), kw
    for w in ((1.0, -0.5, 1.0), (1.0, 1.0, float("nan"))):
        assert call(d=_desc(L), ll=_ll(L, w=w)) == -1 and "class weights must be finite and >= 0" in err(), w
    assert call(d=_desc(L), ll=_ll(L, threshold=float("nan"))) == -1 and "threshold must be finite" in err()
    assert call(d=_desc(L), ll=_ll(L, all_classes=2)) == -1 and "all_classes must be 0 or 1" in err()
    assert call(d=_desc(L, inv=-1.0)) == -1 and "inv_global_batch" in err()
    assert call(d=_desc(L, ls=1.0)) == -1 and "label_smoothing" in err()
    assert call(d=_desc(L, eps=0.0)) == -1 and "clip_eps" in err()
    if entry == "lovasz_coeffs":
        need = lib.usseg_lovasz_ws_bytes(32, 3)
        assert call(d=_desc(L), ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
        assert call(d=_desc(L), ws=None) == -1 and call(d=_desc(L), ws=20) == -1 and "workspace" in err()
        assert call(d=_desc(L), counts=None) == -1 and "counts" in err()
    elif entry == "lovasz_loss_sums":
        for s in (-1.0, float("nan"), float("inf")):
            assert call(d=_desc(L), ov_scale=s) == -1 and "ov_scale must be finite and >= 0" in err(), s
        assert call(d=_desc(L, M=2 * 256 * 80, HW=256 * 80), acc_floats=32 + 16 * 39) == -1 and "a grid of 40 workgroups needs 672 accumulator floats" in err()
        assert call(d=_desc(L), counts=None) == -1 and call(d=_desc(L), acc=None) == -1
    else:
        assert call(d=_desc(L), acc_floats=31) == -1 and "header floats" in err()
        assert call(d=_desc(L), dl=None) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
        assert call(d=_desc(L, lddl=16)) == -1 and "dlogits stride" in err()
        assert call(d=_desc(L, lddl=16, quad_w=3)) == -1 and "quad layout" in err()
        assert call(d=_desc(L, M=0)) == 0                     # nothing to do, nothing launched
