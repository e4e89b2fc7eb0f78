"""Knowledge distillation without a device: the restatement's known answers, ``distill_config``, the third header and the argument checks of
``usseg_distill_loss`` (they return before any launch)."""
import ctypes as C
import math
import os

import pytest
import torch

import distill_restatement as D
import overlap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(2.0, 0.5, 0.5), (1.0, 1.0, 0.0), (4.0, 0.3, 0.7), (0.5, 1.0, 1.0)]


# ------------------------------------------------------------------------------------------------ the restatement
def _case(C_=3, B=2, H=9, W=7):
    logits, y, q = D.inputs(C_, B, H, W)
    return logits, y, q, torch.softmax(logits, -1)


@pytest.mark.parametrize("T,sw,hw", SETTINGS)
def test_the_same_probabilities_on_both_sides_give_no_soft_term(T, sw, hw):
    _, y, _, p = _case()
    assert D.soft_per_pixel(p, p, T).abs().max().item() == 0.0
    assert D.soft_dlogits(p, p, T).abs().max().item() == 0.0
    l, hard, soft = D.loss(p, y, p, T, sw, hw, 0.25)
    assert soft.item() == 0.0 and l.item() == 0.25 * hw * hard.item()


def test_temperature_one_without_a_hard_term_is_p_minus_q_up_to_the_epsilon():
    _, y, q, p = _case()
    scale, sw = 0.25, 0.8
    got = D.at_probs(p, y, q, 1.0, sw, 0.0, scale)["dlogits"]
    # soften(r) at T = 1 is (r + 1e-7) / (1 + C*1e-7): within 2*C*1e-7 absolute of r on each side.  p/(p + 1e-7) is 1 - 1e-7/(p + 1e-7): r_c is off
    # by |pT_c - qT_c| * 1e-7/(p_c + 1e-7) (as large as qT_c itself where p_c is far below 1e-7).  dz_j = r_j - p_j*sum_c r_c carries both.
    pT, qT = D.soften(p, 1.0)[0], D.soften(q, 1.0)[0]
    e = (pT - qT).abs() * D.EPS / (p + D.EPS) + 4 * 3 * D.EPS
    bound = scale * sw * (e + p * e.sum(-1, keepdim=True))
    err = (got - scale * sw * (p - q.double())).abs()
    assert (err <= bound).all() and bound.max().item() < 1e-3 * scale * sw


@pytest.mark.parametrize("T,sw,hw", SETTINGS)
@pytest.mark.parametrize("C_", [3, 2, 4])
def test_the_closed_form_equals_autograd_and_sums_to_zero_over_the_classes(C_, T, sw, hw):
    logits, y, q, _ = _case(C_)
    z = logits.clone().requires_grad_(True)
    p = torch.softmax(z, -1)
    l, _, _ = D.loss(p, y, q, T, sw, hw, 0.25)
    l.backward()
    want = D.at_probs(p.detach(), y, q, T, sw, hw, 0.25)
    scale = max(z.grad.abs().max().item(), 1e-30)
    assert (want["dlogits"] - z.grad).abs().max().item() <= 1e-12 * max(scale, 1.0)
    assert abs(want["loss"] - l.item()) <= 1e-12 * abs(l.item())
    soft = D.soft_dlogits(p.detach(), q, T)
    assert soft.sum(-1).abs().max().item() <= 1e-14 * T                 # a softmax gradient: the classes of a pixel sum to zero
    assert (want["mag"] >= want["dlogits"].abs() * (1 - 1e-12)).all()     # the magnitude dominates what it bounds


def test_finite_differences_in_fp64():
    logits, y, q, _ = _case(3, 1, 3, 2)
    T, sw, hw, scale = 2.0, 0.5, 0.5, 0.5
    f = lambda z: D.loss(torch.softmax(z, -1), y[:1, :3, :2], q[:1, :3, :2], T, sw, hw, scale)[0].item()
    z0 = logits[:1, :3, :2].clone()
    want = D.at_probs(torch.softmax(z0, -1), y[:1, :3, :2], q[:1, :3, :2], T, sw, hw, scale)["dlogits"]
    h = 1e-6
    for idx in [(0, 0, 0, 0), (0, 1, 1, 2), (0, 2, 0, 1)]:
        zp, zm = z0.clone(), z0.clone()
        zp[idx] += h
        zm[idx] -= h
        fd = (f(zp) - f(zm)) / (2 * h)
        assert abs(fd - want[idx].item()) <= 1e-7 * max(1.0, abs(fd)), (idx, fd, want[idx].item())


@pytest.mark.parametrize("C_", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", [(2, 256, 80), (1, 64, 47), (1, 9, 7), (1, 1, 1), (1, 725, 725), (1, 64, 46), (2, 6, 4)])
def test_the_gpu_tests_inputs_leave_no_pixel_at_a_clip_edge(C_, B, H, W):
    """The share of pixels the GPU test leaves out is capped at 1e-3; at its inputs the reference alone leaves out none."""
    logits, y, q = D.inputs(C_, B, H, W)
    p = D.probs32(logits).double()
    n = p / p.sum(-1, keepdim=True)
    rel = 2.0 ** -20
    edge = (((n - R.LO).abs() <= rel * R.LO) | ((n - R.HI).abs() <= rel * R.HI)).any(-1)
    assert int(edge.sum()) == 0


# ------------------------------------------------------------------------------------------------ distill_config
def test_distill_config_defaults_and_refusals():
    from ultrasound_modeling_amd.distill import DISTILL_KEYS, distill_config
    want = {"temperature": 2.0, "soft_weight": 0.5, "hard_weight": 0.5}
    assert distill_config(None) == want and distill_config({}) == want and tuple(want) == DISTILL_KEYS
    assert distill_config({"temperature": 4}) == {**want, "temperature": 4.0}
    assert distill_config({"soft_weight": 0, "hard_weight": 1}) == {**want, "soft_weight": 0.0, "hard_weight": 1.0}
    assert distill_config({"temperature": 0.125})["temperature"] == 0.125 and distill_config({"temperature": 8})["temperature"] == 8.0
    for T in (float("nan"), float("inf"), 0.0, -1.0, 0.1249, 8.001):
        with pytest.raises(ValueError, match="temperature"):
            distill_config({"temperature": T})
    for k in ("soft_weight", "hard_weight"):
        for v in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=k):
                distill_config({k: v})
    with pytest.raises(ValueError, match="both zero"):
        distill_config({"soft_weight": 0.0, "hard_weight": 0.0})
    with pytest.raises(ValueError, match="unknown settings"):
        distill_config({"temperatur": 2.0})
    with pytest.raises(ValueError, match="a dict"):
        distill_config([2.0, 0.5, 0.5])
    with pytest.raises(ValueError, match="number"):
        distill_config({"temperature": "hot"})
    doc = distill_config.__doc__
    assert "nobody has measured" in doc


# ------------------------------------------------------------------------------------------------ the third header and the C ABI
NEW_SYMBOLS = ("usseg_distill_grid", "usseg_distill_loss")


def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def test_the_third_header_parses_and_the_first_is_untouched():
    from ultrasound_modeling_amd import _abi
    L, lib = _lib()
    path = os.path.join(ROOT, "include", "usseg_distill.h")
    assert L.DISTILL_HEADER_PATH == path
    abi = _abi.parse(open(path).read(), path)
    assert tuple(abi.protos) == NEW_SYMBOLS == L.DISTILL_SYMBOLS == tuple(L.DISTILL_ABI.protos)
    assert list(abi.structs) == ["UssegDistillDesc"]
    assert list(abi.consts.items()) == [("USSEG_DISTILL_ACC_FLOATS", 8224), ("USSEG_DISTILL_SETTINGS", 4)]
    assert (L.DISTILL_ACC_FLOATS, L.DISTILL_SETTINGS) == (8224, 4)
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert [(n, t) for n, t in abi.structs["UssegDistillDesc"]._fields_] == [
        ("M", i64), ("HW", i32), ("C", i32), ("lddl", i32), ("quad_w", i32), ("label_smoothing", f32), ("clip_eps", f32), ("inv_global_batch", f32)]
    assert C.sizeof(L.DistillDesc) == 40
    assert abi.protos["usseg_distill_grid"] == (C.c_int, [i64])
    res, args = abi.protos["usseg_distill_loss"]
    assert res == C.c_int and args[1:] == [vp, vp, vp, vp, vp, i64, vp, vp] and args[0]._type_ is abi.structs["UssegDistillDesc"]
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name not in hdr and name not in L.EXPORTED_SYMBOLS and name not in L._PROTOS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == L.DISTILL_ABI.protos[name]            # load() bound the third header's prototypes
    assert (len(L.ABI.protos), len(L.ABI.structs)) == (167, 34) and "usseg_distill" not in hdr
    assert len(L.SCORES_ABI.protos) == 3
    text = open(path).read()
    for phrase in ("softmax_c( log(r_c + 1e-7) / T )", "T^2 * sum_c qT_c * (log qT_c - log pT_c)", "G_c = T * (pT_c - qT_c) / (p_c + 1e-7)",
                   "exactly 0.0", "clamp(ceil(ceil(M/4)/256), 1, 512)", "M == 0 launches no kernel", "every argument is checked BEFORE any launch"):
        assert phrase in text, phrase
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    assert sum("distill.hip" in line.split() for line in mk.splitlines() if line.startswith(("SRCS", "NOPK_SRCS"))) == 2
    assert any(line.startswith("%.o:") and "usseg_distill.h" in line for line in mk.splitlines())
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "DISTILL_SYMBOLS" in entry                                                   # build() looks for the third header's symbols too


def test_the_grid_rule():
    _, lib = _lib()
    for M in (0, 1, 4, 1024, 1025, 2 * 256 * 80, 725 * 725, 1 << 29):
        assert lib.usseg_distill_grid(M) == R.sum_depth(M)[1]
    assert lib.usseg_distill_grid(725 * 725) == 512 and (725 * 725 + 3) // 4 == 131407 and 725 * 725 % 4 == 1


def test_distill_loss_refuses_bad_arguments_before_any_launch():
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(M=64, HW=64, C_=3, lddl=8, quad_w=0, ls=0.1, eps=1e-7, inv=0.5, probs=16, y=16, q=16, settings=16, acc=16, acc_floats=8224, dl=16, desc=True):
        d = L.DistillDesc(M, HW, C_, lddl, quad_w, ls, eps, inv)
        return lib.usseg_distill_loss(C.byref(d) if desc else None, probs, y, q, settings, acc, acc_floats, dl, None)

    assert call(desc=False) == -1 and "distill_loss: null descriptor" in err()
    for c in (0, 5, -1):
        assert call(C_=c) == -1 and "distill_loss: 1 <= C <= 4" in err()
    for kw in (dict(HW=0), dict(M=-64), dict(M=65), dict(HW=-8)):
        assert call(**kw) == -1 and "M must be a non-negative multiple of HW" in err(), kw
    assert call(M=(1 << 29) + 64) == -1 and "more than 2^29 pixels" in err()
    for kw in (dict(probs=None), dict(y=None), dict(q=None), dict(settings=None), dict(acc=None)):
        assert call(**kw) == -1 and "distill_loss: null pointer" in err(), kw
    for kw in (dict(probs=20), dict(y=24), dict(q=8)):
        assert call(**kw) == -1 and "probs, y_true and q must be 16-byte aligned" in err(), kw
    for kw in (dict(settings=18), dict(acc=17)):
        assert call(**kw) == -1 and "4-byte aligned" in err(), kw
    assert call(dl=24) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
    for kw in (dict(quad_w=7, lddl=16), dict(quad_w=-2, lddl=16), dict(quad_w=6, lddl=16), dict(M=15, HW=15, quad_w=2, lddl=16)):   # odd W; negative; 64 % 12; odd H
        assert call(**kw) == -1 and "quad layout needs even H and W" in err(), kw
    for kw in (dict(lddl=16), dict(lddl=4), dict(quad_w=8, lddl=8)):
        assert call(**kw) == -1 and "dlogits stride must be 8 (16 in the quad layout)" in err(), kw
    for inv in (-0.5, float("nan"), float("inf")):
        assert call(inv=inv) == -1 and "inv_global_batch must be finite and >= 0" in err()
    for ls in (-0.1, 1.0, float("nan")):
        assert call(ls=ls) == -1 and "label_smoothing must lie in [0, 1)" in err()
    for eps in (0.0, -1e-7, 1e-9, 0.5, float("nan")):
        assert call(eps=eps) == -1 and "clip_eps must be > 0 and representable below 1 in fp32" in err(), eps
    assert call(acc_floats=32 + 16 * 1 - 1) == -1 and "a grid of 1 workgroups needs 48 accumulator floats" in err()
    assert call(M=2048, HW=64, acc_floats=32 + 16 * 2 - 1) == -1 and "a grid of 2 workgroups needs 64 accumulator floats" in err()


def test_the_model_refuses_contradictory_settings_before_it_builds_anything():
    """The constructor's refusals that need no device: they are raised before the first allocation."""
    from ultrasound_modeling_amd.VisionTransformer import DISTILL_LOSSES, VisionTransformer
    assert DISTILL_LOSSES == ("distill",)
    kw = dict(batch_size=2, img_size=(64, 64), in_channels=1, device="cpu")
    with pytest.raises(ValueError, match="needs teacher="):
        VisionTransformer(loss="distill", **kw)
    for loss in ("cce", "focal"):
        with pytest.raises(ValueError, match="only apply to loss in"):
            VisionTransformer(loss=loss, distill={}, **kw)
        with pytest.raises(ValueError, match="only apply to loss in"):
            VisionTransformer(loss=loss, teacher=object(), **kw)
    for other in (dict(class_factor=[1, 1, 1]), dict(focal_gamma=2), dict(overlap={}), dict(boundary={}), dict(lovasz={}), dict(topk={}), dict(smooth=1.0)):
        with pytest.raises(ValueError, match="do not combine with loss='distill'"):
            VisionTransformer(loss="distill", teacher=object(), **other, **kw)
    with pytest.raises(ValueError, match="temperature"):
        VisionTransformer(loss="distill", teacher=object(), distill={"temperature": 9.0}, **kw)
    with pytest.raises(ValueError, match="unknown settings"):
        VisionTransformer(loss="distill", teacher=object(), distill={"T": 2.0}, **kw)
