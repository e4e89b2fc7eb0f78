"""The class loss (VisionTransformer.my_loss_cat and its focal variant) without a GPU: known answers of the fp64 restatement
(tests/loss_restatement.py), its tie to the committed oracle, finite differences of its gradient, and the argument checks of the three
new C-ABI entry points (each refuses a bad argument with the library's error code and a message of its own before any launch)."""
import ctypes as C
import math

import pytest
import torch

import loss_restatement as R
import usseg_oracle as O

CF = R.CLASS_FACTOR


def _ys(y, C_=3):
    return [v * 0.9 + 0.1 / C_ for v in y]


# ------------------------------------------------------------------------------------------------ known answers, by hand
P1 = [0.7, 0.2, 0.1]
Y1 = [0.0, 1.0, 0.0]


def _one(p, y):
    return torch.tensor(y, dtype=torch.float64).reshape(1, 1, 1, -1), torch.tensor(p, dtype=torch.float64).reshape(1, 1, 1, -1)


def test_my_loss_cat_one_pixel_by_hand():
    y, p = _one(P1, Y1)
    want = -3.0 * sum(CF[c] * _ys(Y1)[c] * math.log(P1[c]) for c in range(3))
    got = R.my_loss_cat(y, p)
    assert tuple(got.shape) == (1, 1) and abs(got.item() - want) <= 1e-14 * abs(want)
    assert abs(R.scalar(y, p, CF, 0.0, 3.0, global_batch=4).item() - want / 4) <= 1e-14 * abs(want)


def test_focal_one_pixel_by_hand():
    y, p = _one(P1, Y1)
    want = -sum(_ys(Y1)[c] * (1 - P1[c]) ** 2 * math.log(P1[c]) for c in range(3))
    got = R.loss_map(y, p, *R.FORMS["focal"])
    assert abs(got.item() - want) <= 1e-14 * abs(want)


def test_weighted_focal_one_pixel_by_hand():
    y, p = _one(P1, Y1)
    want = -3.0 * sum(CF[c] * _ys(Y1)[c] * (1 - P1[c]) ** 1.5 * math.log(P1[c]) for c in range(3))
    got = R.loss_map(y, p, *R.FORMS["weighted_focal"])
    assert abs(got.item() - want) <= 1e-14 * abs(want)


@pytest.mark.parametrize("name", list(R.FORMS))
def test_clipped_probabilities_give_a_finite_loss_and_no_gradient(name):
    """p = 1 and p = 0 are clipped to the fp32 values of 1 - 1e-7 and 1e-7: the loss is finite and its gradient there is zero."""
    w, gamma, factor = R.FORMS[name]
    y, p = _one([1.0, 0.0, 0.25], [0.0, 0.0, 1.0])
    p.requires_grad_(True)
    l = R.loss_map(y, p, w, gamma, factor).sum()
    l.backward()
    ys = _ys([0.0, 0.0, 1.0])
    pc = [R.HI, R.LO, 0.25]
    want = -factor * sum(w[c] * ys[c] * (1 - pc[c]) ** gamma * math.log(pc[c]) for c in range(3))
    assert math.isfinite(l.item()) and abs(l.item() - want) <= 1e-13 * abs(want)
    g = p.grad.reshape(-1)
    assert g[0].item() == 0 and g[1].item() == 0 and g[2].item() != 0
    d2 = factor * w[2] * ys[2] * (gamma * (1 - 0.25) ** (gamma - 1) * math.log(0.25) - (1 - 0.25) ** gamma / 0.25)      # the stated derivative
    assert abs(g[2].item() - d2) <= 1e-13 * abs(d2)
    assert R.LO == float(torch.tensor(1e-7, dtype=torch.float32)) and R.HI == 1.0 - 2.0 ** -23


def test_gamma_zero_equals_the_focal_line_with_exponent_zero():
    g = torch.Generator().manual_seed(5)
    p = torch.softmax(3 * torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64), -1)
    y = torch.softmax(torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64), -1)
    a = R.per_pixel(y, p, CF, 0.0, 3.0)
    b = -3.0 * torch.sum((y * 0.9 + 0.1 / 3) * torch.log(p.clamp(R.LO, R.HI)) * torch.pow(1.0 - p.clamp(R.LO, R.HI), 0.0) * torch.tensor(CF, dtype=torch.float64), -1)
    assert torch.equal(a, b)


def test_unnormalised_probabilities_are_not_divided_by_their_sum():
    """Keras' CategoricalCrossentropy (O.compute_loss) divides by the class sum; my_loss_cat does not: with w = 1/3 and factor 3 the two agree on
    normalised input and differ by sum_c ys*log(S) on input scaled by S."""
    g = torch.Generator().manual_seed(6)
    p = torch.softmax(torch.randn(2, 4, 4, 3, generator=g, dtype=torch.float64), -1)
    y = torch.softmax(torch.randn(2, 4, 4, 3, generator=g, dtype=torch.float64), -1)
    third = [1.0 / 3] * 3
    S = 0.5
    got = R.scalar(y, p * S, third, 0.0, 3.0, 2).item()
    keras = O.compute_loss(y, p * S, 2).item()
    assert abs(keras - O.compute_loss(y, p, 2).item()) <= 1e-12 * abs(keras)            # Keras: the scale drops out
    shift = -math.log(S) * 2 * 4 * 4 / 2                                                 # sum_c ys = 1 per pixel, 32 pixels, / global batch 2
    assert abs(got - (keras + shift)) <= 1e-12 * abs(got) and abs(got - keras) > 1.0


def test_y_true_is_not_modified():
    y, p = _one(P1, Y1)
    y0 = y.clone()
    R.my_loss_cat(y, p)
    R.loss_map(y, p, *R.FORMS["focal"])
    R.from_logits(torch.zeros(1, 1, 1, 3), y, CF, 0.0, 3.0, 1.0)
    assert torch.equal(y, y0)


def test_uniform_weights_tie_the_restatement_to_the_committed_oracle():
    """w = 1/3, factor = 3, gamma = 0 on normalised, unclipped probabilities: both are -sum ys*log p / B."""
    x_, y = O.synthetic_batch(2, 16, 16, 1, seed=3)
    y = y[:, :8, :8]
    g = torch.Generator().manual_seed(7)
    p = torch.softmax(3 * torch.randn(2, 8, 8, 3, generator=g, dtype=torch.float64), -1)
    assert p.min().item() > 1e-6 and p.max().item() < 1 - 1e-6
    a = R.scalar(y, p, [1.0 / 3] * 3, 0.0, 3.0, 4).item()
    b = O.compute_loss(y, p, 4).item()
    assert abs(a - b) <= 1e-12 * abs(b), (a, b)


@pytest.mark.parametrize("name", list(R.FORMS))
def test_finite_differences_of_the_restatement_through_the_softmax(name):
    w, gamma, factor = R.FORMS[name]
    g = torch.Generator().manual_seed(8)
    z = 2 * torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    y = torch.softmax(torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64), -1)
    r = R.from_logits(z, y, w, gamma, factor, 0.25)
    f = lambda t: (R.per_pixel(y, torch.softmax(t, -1), w, gamma, factor).sum() * 0.25).item()
    assert abs(f(z) - r["loss"].item()) <= 1e-14 * abs(r["loss"].item())
    h = 1e-5
    fd = torch.zeros_like(z).reshape(-1)
    for i in range(z.numel()):
        e = torch.zeros(z.numel(), dtype=torch.float64)
        e[i] = h
        fd[i] = (f(z + e.reshape(z.shape)) - f(z - e.reshape(z.shape))) / (2 * h)
    err = (fd.reshape(z.shape) - r["dlogits"]).abs().max().item()
    assert err <= 1e-8 * r["dlogits"].abs().max().item(), err          # central differences: O(h^2) = 1e-10 relative, rounding 1e-16/h
    # the stated derivative d l / d p, inside the clip range
    p = r["probs"]
    ys = y * 0.9 + 0.1 / 3
    wt = torch.tensor(w, dtype=torch.float64)
    stated = 0.25 * factor * wt * ys * (gamma * (1 - p) ** (gamma - 1) * torch.log(p) - (1 - p) ** gamma / p) if gamma else -0.25 * factor * wt * ys / p
    assert ((stated - r["dLdp"]).abs() <= 1e-12 * stated.abs()).all()


def test_the_restatement_keeps_the_gpu_tests_inputs_away_from_the_clip_edges():
    """The inputs of tests/test_gpu_class_loss.py (logits 3*randn with one forced row): only the forced pixel has a probability within 2^-20
    relative of a clip constant, and it is clipped on every class by orders of magnitude (p = 1, e^-80, e^-40)."""
    for C_ in (3, 2, 4):
        logits, y = R.flat_inputs(C_)
        r = R.from_logits(logits, y, *R.form("focal", C_), 0.25)
        edge = r["edge"].clone()
        assert edge[0, 0, 0].item() and r["dLdp"][0, 0, 0].abs().max().item() == 0
        edge[0, 0, 0] = False
        assert int(edge.sum()) == 0


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _cl(L, w=(0.06329, 0.027567, 0.90914), gamma=0.0, factor=3.0):
    w = list(w) + [0.0] * (8 - len(w))
    return L.ClassLoss((C.c_float * 8)(*w), gamma, factor)


def _desc(L, C_=3, M=32, HW=16, ldl=4, lddl=8, kind=2, quad_w=0, eps=1e-7):
    return L.LossDesc(M, HW, C_, ldl, lddl, kind, 0.1, eps, 0.25, quad_w)


def _calls(L, lib):
    """name -> callable(desc-or-C, class loss pointer, **pointer overrides) -> rc, for the three entry points, with non-null dummy pointers
    (never dereferenced: every case fails a check before the launch)."""
    def flat(C_=3, cl=None, d=None, **kw):
        a = dict(logits=16, y_true=16, probs=16, loss=16, dlogits=16)
        a.update(kw)
        d = d if d is not None else _desc(L, C_)
        return lib.usseg_softmax_loss_fwd_bwd_cl(C.byref(d), cl, a["logits"], a["y_true"], a["probs"], a["loss"], a["dlogits"], None)

    def head(C_=3, cl=None, d=None, eps=1e-7, **kw):
        a = dict(x=16, B=1, h=16, w=16, Cin=16, ldx=16, wq=16, bias=16, y_true=16, probs=16, loss=16, dlogits=16)
        a.update(kw)
        return lib.usseg_head_quad_softmax_loss_cl(a["x"], a["B"], a["h"], a["w"], a["Cin"], a["ldx"], a["wq"], a["bias"], C_, a["y_true"], a["probs"],
                                                   a["loss"], a["dlogits"], 0.1, eps, 0.25, cl, None)

    def probs(C_=3, cl=None, d=None, **kw):
        a = dict(probs=16, y_true=16, loss=16)
        a.update(kw)
        d = d if d is not None else _desc(L, C_)
        return lib.usseg_loss_from_probs_cl(C.byref(d), cl, a["probs"], a["y_true"], a["loss"], 0, None)
    return dict(softmax_loss_cl=flat, head_quad_softmax_loss_cl=head, loss_from_probs_cl=probs)


def test_new_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name in ("usseg_softmax_loss_fwd_bwd_cl", "usseg_head_quad_softmax_loss_cl", "usseg_loss_from_probs_cl"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(L.ClassLoss) == 40


@pytest.mark.parametrize("entry", ["softmax_loss_cl", "head_quad_softmax_loss_cl", "loss_from_probs_cl"])
def test_class_loss_entry_points_refuse_bad_arguments_before_any_launch(entry):
    L, lib = _lib()
    call = _calls(L, lib)[entry]
    err = lambda: lib.usseg_last_error().decode()
    assert call(cl=None) == -1 and f"{entry}: null class-loss struct" in err()
    maxc = 4 if entry == "head_quad_softmax_loss_cl" else 8
    for bad_c in (0, maxc + 1):
        assert call(C_=bad_c, cl=C.byref(_cl(L))) == -1 and f"{entry}: 1 <= C <= {maxc}" in err(), bad_c
    for gamma in (0.5, -1.0, 8.5, float("nan"), float("inf")):
        assert call(cl=C.byref(_cl(L, gamma=gamma))) == -1 and f"{entry}: gamma must be 0 or lie in [1, 8]" in err(), gamma
    for factor in (-1.0, float("nan"), float("inf")):
        assert call(cl=C.byref(_cl(L, factor=factor))) == -1 and f"{entry}: factor must be finite and >= 0" in err(), factor
    for w in ((1.0, -0.5, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0)):
        assert call(cl=C.byref(_cl(L, w=w))) == -1 and f"{entry}: class weights must be finite and >= 0" in err(), w
    if entry != "loss_from_probs_cl":
        assert call(cl=C.byref(_cl(L)), y_true=None) == -1 and "dlogits needs y_true" in err()
    if entry != "head_quad_softmax_loss_cl":
        assert call(cl=C.byref(_cl(L)), d=_desc(L, kind=0)) == -1 and f"{entry}: the descriptor must say loss_kind 2" in err()
        assert call(cl=C.byref(_cl(L)), d=_desc(L, eps=0.0)) == -1 and "clip_eps" in err()
    else:
        assert call(cl=C.byref(_cl(L)), eps=0.0) == -1 and "clip_eps" in err()


def test_class_loss_entry_points_keep_the_existing_geometry_checks():
    L, lib = _lib()
    calls = _calls(L, lib)
    err = lambda: lib.usseg_last_error().decode()
    cl = _cl(L, gamma=2.0, factor=1.0)
    assert calls["softmax_loss_cl"](cl=C.byref(cl), d=_desc(L, M=33)) == -1 and "M must be a multiple of HW" in err()
    assert calls["softmax_loss_cl"](cl=C.byref(cl), d=_desc(L, lddl=16)) == -1 and "dlogits stride" in err()
    assert calls["softmax_loss_cl"](cl=C.byref(cl), d=_desc(L, ldl=4, quad_w=4)) == -1 and "quad layout" in err()
    assert calls["softmax_loss_cl"](C_=5, cl=C.byref(cl), d=_desc(L, C_=5, ldl=16, lddl=16, quad_w=4)) == -1 and "1 <= C <= 4" in err()
    assert calls["softmax_loss_cl"](cl=C.byref(cl), logits=None) == -1 and "null pointer" in err()
    assert calls["softmax_loss_cl"](cl=C.byref(cl), loss=None) == -1 and "loss pointer required" in err()
    assert calls["loss_from_probs_cl"](cl=C.byref(cl), d=_desc(L, M=33)) == -1 and "M must be a multiple of HW" in err()
    assert calls["loss_from_probs_cl"](cl=C.byref(cl), probs=None) == -1 and "null pointer" in err()
    assert calls["head_quad_softmax_loss_cl"](cl=C.byref(cl), ldx=12) == -1 and "bad arguments" in err()
    assert calls["head_quad_softmax_loss_cl"](cl=C.byref(cl), loss=None) == -1 and "loss pointer required" in err()
    assert calls["head_quad_softmax_loss_cl"](cl=C.byref(cl), Cin=40, ldx=40) == -2 and "no fused kernel" in err()      # unsupported width: nothing launched
    assert lib.usseg_softmax_loss_fwd_bwd_cl(None, C.byref(cl), 16, 16, 16, 16, 16, None) == -1 and "null descriptor" in err()
    # the existing entry points still refuse loss_kind 2: its parameters only travel through the new ones
    d = _desc(L, kind=2)
    assert lib.usseg_softmax_loss_fwd_bwd(C.byref(d), 16, 16, None, 16, 16, 16, None) == -1
    assert lib.usseg_loss_from_probs(C.byref(d), 16, 16, None, 16, None) == -1


def test_python_surface_refuses_bad_class_losses():
    from ultrasound_modeling_amd import ops
    for kw in (dict(w=[1.0] * 9), dict(w=[]), dict(w=[1, 1, 1], gamma=0.5), dict(w=[1, 1, 1], gamma=9), dict(w=[1, -1, 1]),
               dict(w=[1, 1, 1], factor=float("nan"))):
        with pytest.raises(ValueError):
            ops.class_loss(**kw)
    cl = ops.class_loss(R.CLASS_FACTOR, 0.0, 3.0)
    assert [round(v, 6) for v in list(cl.w)[:3]] == [0.06329, 0.027567, 0.90914] and cl.gamma == 0.0 and cl.factor == 3.0


def test_drivers_take_a_loss_keyword():
    import inspect
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    from ultrasound_modeling_amd.VisionTransformer import LOSSES, VisionTransformer
    assert LOSSES == ("cce", "my_loss_cat", "focal")
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main, VisionTransformer.__init__, TBI_TransUNet.VisionTransformer.__init__):
        assert inspect.signature(fn).parameters["loss"].default == "cce", fn
