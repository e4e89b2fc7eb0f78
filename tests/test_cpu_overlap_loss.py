"""The region-overlap losses (soft Dice / Tversky, optionally plus CCE; usseg.h UssegOverlapLoss) without a GPU: known answers of the fp64
restatement (tests/overlap_restatement.py), its tie to the committed oracle's CCE, finite differences of its gradient, the constructor's
refusals, the C ABI (struct layout, exported symbols, every argument check of the two entry points before any launch) and
``metrics.dice_per_class``."""
import ctypes as C
import inspect
import math

import pytest
import torch

import overlap_restatement as R
import usseg_oracle as O


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("loss", ["dice", "tversky"])
def test_a_perfect_one_hot_prediction_has_every_index_one_and_no_loss(loss):
    g = torch.Generator().manual_seed(1)
    y = torch.nn.functional.one_hot(torch.randint(0, 3, (2, 5, 7), generator=g), 3).double()
    cfg = R.config(loss, power=2.0)
    I, P, Y = R.sums(y, y)
    _, _, T = R.tversky(I, P, Y, cfg["alpha"], cfg["beta"], cfg["smooth"])
    # exact for a = b = 0.5; 0.3 and 0.7 are not fp64 numbers, so (1-a-b)*I + a*P + b*Y is I only to a few units in the last place
    ulp = 0.0 if loss == "dice" else 2.0 ** -50
    assert ((T - 1.0).abs() <= ulp).all()
    assert 0.0 <= R.loss(y, y, cfg).item() <= ulp ** 2


def test_two_pixels_two_classes_by_hand():
    """p = [[0.8, 0.2], [0.4, 0.6]], y = [[1, 0], [0, 1]], Tversky a = 0.3, b = 0.7, s = 1, w = [0.25, 0.75], g = 1, ov_weight 2, ov_scale 0.5."""
    p = torch.tensor([[0.8, 0.2], [0.4, 0.6]], dtype=torch.float64)
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    cfg = R.config("tversky", 2, w=[0.25, 0.75], ov_weight=2.0)
    I, P, Y = R.sums(p, y)
    assert I.tolist() == [0.8, 0.6] and torch.allclose(P, torch.tensor([1.2, 0.8], dtype=torch.float64), rtol=0, atol=1e-15) and Y.tolist() == [1.0, 1.0]
    N, D, T = R.tversky(I, P, Y, 0.3, 0.7, 1.0)
    # a + b = 1: D = 0.3*P + 0.7*Y + 1
    d0, d1 = 0.3 * 1.2 + 0.7 + 1.0, 0.3 * 0.8 + 0.7 + 1.0
    assert abs(D[0].item() - d0) < 1e-15 and abs(D[1].item() - d1) < 1e-15
    assert abs(T[0].item() - 1.8 / d0) < 1e-15 and abs(T[1].item() - 1.6 / d1) < 1e-15
    want = 2.0 * 0.5 * (0.25 * (1 - 1.8 / d0) + 0.75 * (1 - 1.6 / d1))
    assert abs(R.loss(p, y, cfg, ov_scale=0.5).item() - want) < 1e-15
    A, B = R.coefficients(I, P, Y, cfg, ov_scale=0.5)
    k0, k1 = 2.0 * 0.5 * 0.25, 2.0 * 0.5 * 0.75
    assert abs(A[0].item() + k0 / d0) < 1e-15 and abs(A[1].item() + k1 / d1) < 1e-15          # (1-a-b) = 0: A = -k/D
    assert abs(B[0].item() - k0 * 0.3 * 1.8 / d0 ** 2) < 1e-15 and abs(B[1].item() - k1 * 0.3 * 1.6 / d1 ** 2) < 1e-15
    # the stated gradient equals autograd at the probabilities
    pp = p.clone().requires_grad_(True)
    R.loss(pp, y, cfg, ov_scale=0.5).backward()
    assert torch.allclose(pp.grad, A * y + B, rtol=1e-13, atol=0)


def test_alpha_beta_one_half_is_the_textbook_dice_with_smoothing_two_s():
    g = torch.Generator().manual_seed(2)
    p = torch.softmax(torch.randn(2, 6, 5, 3, generator=g, dtype=torch.float64), -1)
    y = torch.softmax(2 * torch.randn(2, 6, 5, 3, generator=g, dtype=torch.float64), -1)
    s = 0.75
    I, P, Y = R.sums(p, y)
    _, _, T = R.tversky(I, P, Y, 0.5, 0.5, s)
    textbook = (2 * I + 2 * s) / (P + Y + 2 * s)
    assert torch.allclose(T, textbook, rtol=1e-14, atol=0)
    want = ((1.0 - textbook) / 3).sum().item()
    assert abs(R.loss(p, y, R.config("dice", smooth=s)).item() - want) <= 1e-14 * want


def test_the_cce_term_alone_is_the_oracles_compute_loss():
    _x, y = O.synthetic_batch(2, 16, 16, 1, seed=3)
    y = y[:, :8, :8]
    g = torch.Generator().manual_seed(7)
    p = torch.softmax(3 * torch.randn(2, 8, 8, 3, generator=g, dtype=torch.float64), -1)
    a = R.loss(p, y, R.config("dice_ce", ov_weight=0.0, ce_weight=1.0), inv_global_batch=0.25).item()
    b = O.compute_loss(y, p, 4).item()
    assert abs(a - b) <= 1e-12 * abs(b), (a, b)
    both = R.loss(p, y, R.config("dice_ce"), inv_global_batch=0.25).item()
    assert abs(both - (b + R.loss(p, y, R.config("dice")).item())) <= 1e-12 * both


@pytest.mark.parametrize("C_", [2, 3, 4])
@pytest.mark.parametrize("power", [1.0, 2.0])
@pytest.mark.parametrize("loss", ["tversky", "dice_ce"])
def test_finite_differences_of_the_restatement_through_the_softmax(C_, power, loss):
    g = torch.Generator().manual_seed(8 + C_)
    z = 2 * torch.randn(2, 3, 3, C_, generator=g, dtype=torch.float64)
    y = torch.softmax(torch.randn(2, 3, 3, C_, generator=g, dtype=torch.float64), -1)
    cfg = R.config(loss, C_, power=power, w=[0.2 + 0.3 * c for c in range(C_)])
    r = R.from_logits(z, y, cfg, 0.25, 0.5)
    f = lambda t: R.loss(torch.softmax(t, -1), y, cfg, 0.25, 0.5).item()
    assert abs(f(z) - r["loss"].item()) <= 1e-14 * abs(r["loss"].item())
    h = 1e-5
    fd = torch.zeros(z.numel(), dtype=torch.float64)
    for i in range(z.numel()):
        e = torch.zeros(z.numel(), dtype=torch.float64)
        e[i] = h
        fd[i] = (f(z + e.reshape(z.shape)) - f(z - e.reshape(z.shape))) / (2 * h)
    err = (fd.reshape(z.shape) - r["dlogits"]).abs().max().item()
    assert err <= 1e-8 * r["dlogits"].abs().max().item(), err          # central differences: O(h^2) = 1e-10 relative, rounding 1e-16/h
    # the stated form: dlogit_j = p_j*(G_j - sum_c p_c*G_c), G = A*y + B (+ the CCE gradient, here by autograd)
    G = r["A"] * y + r["B"]
    if cfg["ce_weight"]:
        pc = r["probs"].clone().requires_grad_(True)
        (0.25 * R.cce_per_pixel(pc, y).sum()).backward()
        G = G + pc.grad
    stated = r["probs"] * (G - (G * r["probs"]).sum(-1, keepdim=True))
    assert ((stated - r["dlogits"]).abs() <= 1e-12 * r["mag"]).all()


def test_the_gpu_tests_inputs_stay_away_from_the_cce_clip_edges():
    """Logits from N(0, 2^2): no normalised probability of tests/test_gpu_overlap_loss.py's inputs lies within 2^-20 relative of a clip constant,
    so its dice_ce cases leave no pixel out."""
    for C_ in (2, 3, 4):
        for B, H, W in ((2, 256, 80), (1, 64, 47), (1, 9, 7)):
            logits, y = R.inputs(C_, B, H, W)
            q = torch.softmax(logits, -1)
            rel = 2.0 ** -20
            edge = ((q - R.LO).abs() <= rel * R.LO) | ((q - R.HI).abs() <= rel * R.HI)
            assert int(edge.sum()) == 0
            assert q.min().item() > R.LO and q.max().item() < R.HI


def test_sum_depth_follows_the_grid_rule():
    assert R.sum_depth(63) == (4 + 6 + 2 + 1 + 4 + 1, 1)
    assert R.sum_depth(2 * 256 * 80) == (4 + 6 + 2 + 3 + 4 + 1, 40)
    assert R.sum_depth(1 << 20) == (8 + 6 + 2 + 32 + 4 + 1, 512)
    from ultrasound_modeling_amd import ops
    for M in (0, 1, 63, 1024, 1025, 64 * 47, 2 * 256 * 80, 139264, 552960, 1 << 20):
        assert ops.overlap_loss_grid(M) == R.sum_depth(M)[1], M


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_refuses_bad_overlap_losses():
    from ultrasound_modeling_amd import ops
    for kw in (dict(class_weight=[1.0] * 5), dict(class_weight=[]), dict(class_weight=[1, 1, 1], power=0.5), dict(class_weight=[1, 1, 1], power=4.5),
               dict(class_weight=[1, -1, 1]), dict(class_weight=[1, 1, 1], smooth=0.0), dict(class_weight=[1, 1, 1], smooth=float("nan")),
               dict(class_weight=[1, 1, 1], alpha=-0.1), dict(class_weight=[1, 1, 1], beta=float("inf")), dict(class_weight=[1, 1, 1], ov_weight=-1.0),
               dict(class_weight=[1, 1, 1], power=float("nan")), dict(class_weight=[1, 1, 1], ov_weight=0.0, ce_weight=0.0)):
        with pytest.raises(ValueError):
            ops.overlap_loss(**kw)
    ol = ops.overlap_loss([0.2, 0.3, 0.5], 0.3, 0.7, 2.0, 1.5, 0.25, 0.75)
    got = [round(v, 6) for v in list(ol.w)[:3]] + [round(v, 6) for v in (ol.alpha, ol.beta, ol.smooth, ol.power, ol.ov_weight, ol.ce_weight)]
    assert got == [0.2, 0.3, 0.5, 0.3, 0.7, 2.0, 1.5, 0.25, 0.75]


def test_overlap_config_defaults_and_refusals():
    from ultrasound_modeling_amd.VisionTransformer import LOSSES, OVERLAP_LOSSES, overlap_config
    assert LOSSES == ("cce", "my_loss_cat", "focal") and OVERLAP_LOSSES == ("dice", "tversky", "dice_ce")
    f = lambda ol: (round(ol.alpha, 6), round(ol.beta, 6), ol.smooth, ol.power, ol.ov_weight, ol.ce_weight)
    assert f(overlap_config("dice", 3, None)) == (0.5, 0.5, 1.0, 1.0, 1.0, 0.0)
    assert f(overlap_config("tversky", 3, None)) == (0.3, 0.7, 1.0, 1.0, 1.0, 0.0)
    assert f(overlap_config("dice_ce", 3, None)) == (0.5, 0.5, 1.0, 1.0, 1.0, 1.0)
    assert [round(v, 6) for v in list(overlap_config("dice", 4, None).w)[:4]] == [0.25] * 4
    ol = overlap_config("tversky", 2, dict(alpha=0.6, beta=0.4, smooth=0.5, power=2, class_weight=[0.1, 0.9], ov_weight=3))
    assert f(ol) == (0.6, 0.4, 0.5, 2.0, 3.0, 0.0) and [round(v, 6) for v in list(ol.w)[:2]] == [0.1, 0.9]
    for loss, cfg in (("dice", dict(alpha=0.3)), ("dice_ce", dict(beta=0.7)), ("dice", dict(ce_weight=1.0)), ("tversky", dict(ce_weight=0.5)),
                      ("dice_ce", dict(ce_weight=0.0)), ("dice", dict(gamma=2.0)), ("dice", dict(class_weight=[0.5, 0.5])),
                      ("dice", dict(power=0.5)), ("tversky", dict(alpha=-1.0)), ("dice", dict(smooth=0.0)), ("dice", dict(ov_weight=0.0))):
        with pytest.raises(ValueError):
            overlap_config(loss, 3, cfg)


def test_drivers_and_constructors_take_the_overlap_settings():
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main, VisionTransformer.__init__, TBI_TransUNet.VisionTransformer.__init__):
        par = inspect.signature(fn).parameters
        assert par["loss"].default == "cce" and par["overlap"].default is None, fn
    with pytest.raises(SystemExit):
        MainParallel._cli(["a.npy", "b.npy", "--loss", "hinge"])
    from ultrasound_modeling_amd.VisionTransformer import overlap_settings
    assert overlap_settings("dice", None) == {} and overlap_settings("cce", None) is None and overlap_settings("dice", dict(smooth=2.0)) == dict(smooth=2.0)


def test_constructor_refusals_come_before_any_device_work():
    """Each of these raises ValueError from the argument checks at the top of the constructor, GPU or not."""
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for kw in (dict(loss="hinge"), dict(loss="dice"), dict(loss="tversky"), dict(loss="dice_ce"), dict(loss="cce", overlap=dict(smooth=2.0)), dict(loss="focal", smooth=2.0), dict(loss="dice", overlap={}, class_factor=[1, 1, 1]),
               dict(loss="dice", overlap={}, focal_gamma=2.0), dict(loss="dice", overlap=dict(smooth=2.0), power=2.0), dict(loss="dice", alpha=0.3),
               dict(loss="tversky", overlap=dict(ce_weight=1.0)), dict(loss="dice_ce", ce_weight=0.0), dict(loss="dice", power=5.0),
               dict(loss="dice", num_classes=2, class_weight=[1, 1, 1])):
        with pytest.raises(ValueError):
            VisionTransformer(2, (64, 64), in_channels=1, **kw)
        with pytest.raises(ValueError):
            TransUNet((64, 64), batch_size=2, in_channels=1, **kw)
    for kw in (dict(loss="dice", smoothing=2.0), dict(loss="dice", overlap={}, bogus=1), dict(loss="cce", bogus=1)):      # a stray keyword is a TypeError, first
        with pytest.raises(TypeError):
            VisionTransformer(2, (64, 64), in_channels=1, **kw)
        with pytest.raises(TypeError):
            TransUNet((64, 64), batch_size=2, in_channels=1, **kw)
    for fn in (VisionTransformer.__init__, TransUNet.__init__):                      # explicit keywords: the signatures stay closed
        par = inspect.signature(fn).parameters
        assert all(par[k].default is None and par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in
                   ("alpha", "beta", "smooth", "power", "class_weight", "ce_weight", "ov_weight"))
        assert not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in par.values())


def test_the_three_drivers_reports_keep_the_references_five_lines_in_order():
    """Source-level, without a GPU (tests/test_gpu_overlap_loss.py runs them): each driver's ``test`` prints loss, IoU, f1, precision, recall in
    that order, and the per-class Dice line after them."""
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    for fn in (MainNumpy.Process.test, MainParallel.Process.test, TBI_TransUNet.test):
        src = inspect.getsource(fn)
        pos = [src.index(f'"{label} = {{}}"') for label in ("loss", "IoU", "f1", "precision", "recall", "dice per class")]
        assert pos == sorted(pos), fn


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _ol(L, w=(0.2, 0.3, 0.5), alpha=0.5, beta=0.5, smooth=1.0, power=1.0, ov_weight=1.0, ce_weight=1.0):
    w = list(w) + [0.0] * (8 - len(w))
    return L.OverlapLoss((C.c_float * 8)(*w), alpha, beta, smooth, power, ov_weight, ce_weight)


def _desc(L, C_=3, M=32, HW=16, lddl=8, quad_w=0, eps=1e-7, ls=0.1, inv=0.25):
    return L.LossDesc(M, HW, C_, C_, lddl, 0, ls, eps, inv, quad_w)


def test_struct_layout_and_exported_symbols():
    L, lib = _lib()
    assert C.sizeof(L.OverlapLoss) == 56
    off = {n: getattr(L.OverlapLoss, n).offset for n, _ in L.OverlapLoss._fields_}
    assert off == dict(w=0, alpha=32, beta=36, smooth=40, power=44, ov_weight=48, ce_weight=52)
    for name in ("usseg_overlap_loss_sums", "usseg_overlap_loss_bwd", "usseg_overlap_loss_grid"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    from ultrasound_modeling_amd import ops
    assert ops.OVERLAP_ACC_FLOATS == 32 + 16 * 512
    hdr = open(__file__.replace("tests/test_cpu_overlap_loss.py", "include/usseg.h")).read()
    assert f"#define USSEG_OVERLAP_ACC_FLOATS {ops.OVERLAP_ACC_FLOATS} " in hdr


@pytest.mark.parametrize("entry", ["overlap_loss_sums", "overlap_loss_bwd"])
def test_entry_points_refuse_bad_arguments_before_any_launch(entry):
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(d=None, ol=0, probs=16, y_true=16, acc=16, acc_floats=L_ACC, dl=16, ov_scale=1.0):
        d = C.byref(d) if d is not None else None
        ol = C.byref(_ol(L)) if ol == 0 else (None if ol is None else C.byref(ol))
        if entry == "overlap_loss_sums":
            return lib.usseg_overlap_loss_sums(d, ol, ov_scale, probs, y_true, acc, acc_floats, None)
        return lib.usseg_overlap_loss_bwd(d, ol, probs, y_true, acc, acc_floats, dl, None)

    assert call(d=None) == -1 and f"{entry}: null descriptor" in err()
    assert call(d=_desc(L), ol=None) == -1 and f"{entry}: null overlap-loss struct" in err()
    for kw in (dict(probs=None), dict(y_true=None), dict(acc=None)):
        assert call(d=_desc(L), **kw) == -1 and f"{entry}: null pointer" in err(), kw
    for bad_c in (0, 5):
        assert call(d=_desc(L, C_=bad_c)) == -1 and f"{entry}: 1 <= C <= 4" in err()
    for d in (_desc(L, M=33), _desc(L, HW=0), _desc(L, M=-16)):
        assert call(d=d) == -1 and "M must be a non-negative multiple of HW" in err()
    assert call(d=_desc(L, M=(1 << 29) + 16)) == -1 and "more than 2^29 pixels" in err()
    for kw in (dict(probs=20), dict(y_true=24)):
        assert call(d=_desc(L), **kw) == -1 and "16-byte aligned" in err(), kw
    for kw in (dict(alpha=-0.5), dict(beta=float("nan")), dict(alpha=float("inf"))):
        assert call(d=_desc(L), ol=_ol(L, **kw)) == -1 and "alpha and beta must be finite and >= 0" in err(), kw
    for s in (0.0, -1.0, float("nan"), float("inf")):
        assert call(d=_desc(L), ol=_ol(L, smooth=s)) == -1 and "smooth must be finite and > 0" in err(), s
    for g in (0.5, 0.0, 4.5, float("nan")):
        assert call(d=_desc(L), ol=_ol(L, power=g)) == -1 and "power must lie in [1, 4]" in err(), g
    for kw in (dict(ov_weight=-1.0), dict(ce_weight=float("nan")), dict(ov_weight=float("inf"))):
        assert call(d=_desc(L), ol=_ol(L, **kw)) == -1 and "ov_weight and ce_weight must be finite and >= 0" in err(), kw
    for w in ((1.0, -0.5, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        assert call(d=_desc(L), ol=_ol(L, w=w)) == -1 and "class weights must be finite and >= 0" in err(), w
    for inv in (-1.0, float("nan")):
        assert call(d=_desc(L, inv=inv)) == -1 and "inv_global_batch" in err()
    assert call(d=_desc(L, ls=1.0)) == -1 and "label_smoothing" in err()
    assert call(d=_desc(L, eps=0.0)) == -1 and "clip_eps" in err()
    assert call(d=_desc(L), acc_floats=31) == -1 and "header floats" in err()
    if entry == "overlap_loss_sums":
        for s in (-1.0, float("nan"), float("inf")):
            assert call(d=_desc(L), ov_scale=s) == -1 and "ov_scale must be finite and >= 0" in err(), s
        # a grid with more workgroups than the accumulator has rows: 2 * 256 * 80 pixels are 40 workgroups
        assert call(d=_desc(L, M=2 * 256 * 80, HW=256 * 80), acc_floats=32 + 16 * 39) == -1 and "a grid of 40 workgroups needs 672 accumulator floats" in err()
    else:
        assert call(d=_desc(L), dl=None) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
        assert call(d=_desc(L), dl=24) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
        assert call(d=_desc(L, lddl=16)) == -1 and "dlogits stride" in err()
        assert call(d=_desc(L, lddl=8, quad_w=4)) == -1 and "dlogits stride" in err()
        assert call(d=_desc(L, lddl=16, quad_w=3)) == -1 and "quad layout" in err()
        assert call(d=_desc(L, M=30, HW=15, lddl=16, quad_w=6)) == -1 and "quad layout" in err()
        assert call(d=_desc(L, M=0)) == 0                     # nothing to do, nothing launched


L_ACC = 8224


# ------------------------------------------------------------------------------------------------ per-class Dice of the validation report
def _counts(cm, head=(0, 0, 0, 0, 0, 0), invalid=0):
    nc = len(cm)
    c = list(head) + [v for row in cm for v in row] + [invalid]
    return torch.tensor(c + [0] * (23 - len(c)), dtype=torch.int64)


def test_dice_per_class_against_hand_counts():
    from ultrasound_modeling_amd.metrics import dice_per_class
    cm = [[50, 3, 2], [4, 30, 1], [6, 0, 4]]                  # cm[true][pred]
    d = dice_per_class(_counts(cm))
    assert d == [2 * 50 / (55 + 60), 2 * 30 / (35 + 33), 2 * 4 / (10 + 7)]
    assert dice_per_class(_counts([[5, 1], [2, 8]]), 2) == [10 / (6 + 7), 16 / (10 + 9)]


def test_dice_per_class_of_an_empty_class_is_zero_not_nan():
    from ultrasound_modeling_amd.metrics import dice_per_class
    d = dice_per_class(_counts([[7, 2, 0], [1, 9, 0], [0, 0, 0]]))
    assert d[2] == 0.0 and all(math.isfinite(v) for v in d)
    assert dice_per_class(_counts([[0] * 3] * 3)) == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        dice_per_class(_counts([[1, 0, 0], [0, 1, 0], [0, 0, 1]], invalid=2))
    with pytest.raises(ValueError):
        dice_per_class(_counts([[1]]), 5)


def test_counts_to_metrics_is_unchanged_on_the_same_counters():
    from ultrasound_modeling_amd.metrics import counts_to_metrics, dice_per_class
    cm = [[50, 3, 2], [4, 30, 1], [6, 0, 4]]
    c = _counts(cm, head=(84, 16, 11, 5, 2, 3))
    before = c.clone()
    m = counts_to_metrics(c)
    dice_per_class(c)
    assert torch.equal(c, before)
    assert list(m) == ["precision", "recall", "f1", "c2_precision", "c2_recall", "c2_f1", "mean_iou"]
    p, r = 84 / 100, 84 / 95
    iou = (50 / (55 + 60 - 50) + 30 / (35 + 33 - 30) + 4 / (10 + 7 - 4)) / 3
    assert m["precision"] == p and m["recall"] == r and m["f1"] == 2 * p * r / (p + r)
    assert m["c2_precision"] == 5 / 7 and m["c2_recall"] == 5 / 8 and abs(m["mean_iou"] - iou) < 1e-15
