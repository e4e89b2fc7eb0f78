"""Knowledge distillation on the device: ``usseg_distill_loss`` element by element against tests/distill_restatement.py, its reproducible
sums, and the model hook (``VisionTransformer(loss="distill", teacher=...)``): eager, replayed from a graph, saved and loaded, two ranks.

The per-element bound.  dlogits is ONE bf16 rounding of p_j*(G_j - sum_c p_c*G_c); the sibling files bound the fp32 arithmetic in front of it
and that rounding together by c = 4 units of bf16 (U_BF16) times the magnitude of the terms.  The softening here uses logf / expf (documented
within 1 ulp, csrc/distill.hip): an exponent s_c = logf(p_c + 1e-7)/T reaches 129 at T = 1/8 and 32 at the smallest T tested (0.5), three
roundings put it off by at most 3 ulp(32) = 3 * 2^-18, which is the RELATIVE error of pT_c and qT_c; the quotient by (p_c + 1e-7), the products
with T and the weights and the sum with the hard term add fewer than 8 roundings of 2^-24.  Together below 2^-16 of the terms' magnitude: under
a hundredth of one bf16 unit (2^-9), so c stays the siblings' 4.0.
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distill_restatement as D
import overlap_restatement as R
from route_probe import U_BF16, assert_elementwise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

SETTINGS = [(2.0, 0.5, 0.5), (1.0, 1.0, 0.0), (4.0, 0.3, 0.7), (0.5, 1.0, 1.0)]
# row: 40 workgroups; three, the last partly idle; 63 pixels (a partial last group); one pixel; 131 407 groups for the 131 072 threads of the
# largest grid (some threads take a second group) with M % 4 == 1
ROW_SHAPES = [(2, 256, 80), (1, 64, 47), (1, 9, 7), (1, 1, 1), (1, 725, 725)]
QUAD_SHAPES = [(2, 256, 80), (1, 64, 46), (2, 6, 4)]
ALL_SETTINGS_AT = {(1, 9, 7), (1, 1, 1), (2, 6, 4)}
INV = 0.25


def _cases(shapes):
    return [(shp, C, s) for shp in shapes for C in (3, 2, 4) for s in (SETTINGS if shp in ALL_SETTINGS_AT else SETTINGS[:1])]


def _ids(cases):
    return [f"{b}x{h}x{w}-C{C}-T{s[0]}" for (b, h, w), C, s in cases]


def _table(s):
    return torch.tensor(list(s) + [0.0], dtype=torch.float32, device=DEV)


def _launch(pd, yd, qd, settings, quad, C, B, H, W, acc=None, grad=True):
    from ultrasound_modeling_amd import ops
    import test_gpu_overlap_loss as OL
    acc = torch.zeros(ops.DISTILL_ACC_FLOATS, device=DEV) if acc is None else acc
    dl = None
    if grad:      # pre-filled with NaN: every element must be written
        dl = torch.full(OL._to_quad_shape(B, H, W) if quad else (B, H, W, 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.distill_loss(pd, yd, qd, settings, acc, dl, HW=H * W, C_classes=C, inv_global_batch=INV, quad_w=W if quad else 0)
    torch.cuda.synchronize()
    return acc, dl


def _inputs(C, B, H, W):
    logits, y, q = D.inputs(C, B, H, W)
    p32 = D.probs32(logits)
    return p32, y, q, p32.to(DEV), y.float().to(DEV), q.to(DEV)


def _classes(dl, quad, C):
    """-> the C class channels [B,H,W,C] after checking that every element was written and the pad channels are exactly zero."""
    import test_gpu_overlap_loss as OL
    d = OL._from_quad(dl.float()) if quad else dl.float()
    assert not torch.isnan(d).any()
    if d.shape[-1] > C:
        assert d[..., C:].abs().max().item() == 0
    return d[..., :C]


def _check(what, acc, dl, quad, C, p32, y, q, s):
    T, sw, hw = s
    want = D.at_probs(p32, y, q, T, sw, hw, INV)
    got = acc[:8].double().cpu()
    size = hw * abs(want["hard"]) + sw * abs(want["soft"])
    print(f"\n  {what}: loss {got[0].item():.7f} vs {want['loss']:.7f}; hard {got[2].item():.6f} vs {want['hard']:.6f}; soft {got[3].item():.6f} vs "
          f"{want['soft']:.6f}", end="")
    assert abs(got[0].item() - want["loss"]) <= 1e-5 * INV * size
    assert abs(got[4].item() + got[5].item() - got[0].item()) <= 2.0 ** -23 * abs(got[0].item())        # the two reported terms are the loss
    both = abs(want["hard"]) + abs(want["soft"])
    assert abs(got[2].item() - want["hard"]) <= 1e-5 * both and abs(got[3].item() - want["soft"]) <= 1e-5 * both
    d = _classes(dl, quad, C)
    skip = want["edge"]
    n_skip = int(skip.sum())
    print(f"; {n_skip} of {skip.numel()} pixels at a clip edge left out", end="")
    assert n_skip <= 1e-3 * skip.numel()
    keep = ~skip
    tiny = 2.0 ** -20 * INV * (hw + sw * T)
    assert_elementwise(d.double().cpu()[keep], want["dlogits"][keep], want["mag"][keep], U_BF16, 4.0, tiny=tiny, what=what)


# ------------------------------------------------------------------------------------------------ the kernel
ROW_CASES, QUAD_CASES = _cases(ROW_SHAPES), _cases(QUAD_SHAPES)


@pytest.mark.parametrize("shape,C,s", ROW_CASES, ids=_ids(ROW_CASES))
def test_row_layout_per_element_and_the_sums_bit_for_bit_over_three_calls(shape, C, s):
    from ultrasound_modeling_amd import ops
    B, H, W = shape
    p32, y, q, pd, yd, qd = _inputs(C, B, H, W)
    assert ops.distill_grid(B * H * W) == R.sum_depth(B * H * W)[1]
    acc, runs = None, []
    for _ in range(3):
        acc, dl = _launch(pd, yd, qd, _table(s), False, C, B, H, W, acc=acc)
        assert acc[1].item() == 0                                  # the ticket is back at zero: no per-call zeroing
        runs.append((acc[:32].cpu().clone(), dl.view(torch.int16).cpu().clone()))
    assert all(torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]) for r in runs[1:])
    _check(f"row C={C} {B}x{H}x{W} {s}", acc, dl, False, C, p32, y, q, s)


@pytest.mark.parametrize("shape,C,s", QUAD_CASES, ids=_ids(QUAD_CASES))
def test_quad_layout_per_element(shape, C, s):
    B, H, W = shape
    p32, y, q, pd, yd, qd = _inputs(C, B, H, W)
    acc, dl = _launch(pd, yd, qd, _table(s), True, C, B, H, W)
    assert acc[1].item() == 0
    _check(f"quad C={C} {B}x{H}x{W} {s}", acc, dl, True, C, p32, y, q, s)
    acc0, none = _launch(pd, yd, qd, _table(s), True, C, B, H, W, grad=False)      # the loss alone: the same sums
    assert none is None and torch.equal(acc0[:6], acc[:6])


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("C", [3, 2, 4])
def test_the_teacher_equal_to_the_student_gives_exact_zeros(C, quad):
    B, H, W = 2, 64, 46
    p32, y, q, pd, yd, qd = _inputs(C, B, H, W)
    for T in (2.0, 0.5, 4.0):
        acc, dl = _launch(pd, yd, pd.clone(), _table((T, 0.5, 0.5)), quad, C, B, H, W)
        assert acc[3].item() == 0.0 and acc[5].item() == 0.0 and acc[0].item() == acc[4].item() and acc[0].item() > 0
        acc0, dl0 = _launch(pd, yd, qd, _table((T, 0.0, 0.5)), quad, C, B, H, W)
        assert torch.equal(dl.view(torch.int16), dl0.view(torch.int16))
        assert acc0[0].item() == acc[0].item()


@pytest.mark.parametrize("quad", [False, True])
def test_no_soft_weight_equals_the_existing_cce_launch(quad):
    """soft_weight = 0, hard_weight = 1: the loss and dlogits of the existing loss_kind 0 launch on the same logits (and ``loss_from_probs``)."""
    from ultrasound_modeling_amd import ops
    import test_gpu_overlap_loss as OL
    C, B, H, W = 3, 2, 64, 46
    logits, y, q = D.inputs(C, B, H, W)
    yd = y.float().to(DEV)
    probs = torch.empty(B, H, W, C, device=DEV)
    loss0 = torch.zeros(ops.ACC_FLOATS, device=DEV)
    if quad:
        lq = torch.zeros(B, H // 2, W // 2, 16)
        for a in range(2):
            for b in range(2):
                lq[..., 4 * (a * 2 + b):4 * (a * 2 + b) + C] = logits.float()[:, a::2, b::2, :]
        lg, dl0 = lq.to(DEV), ops.new_act(B, H // 2, W // 2, 16, DEV)
    else:
        lg = torch.zeros(B, H, W, 4)
        lg[..., :C] = logits.float()
        lg, dl0 = lg.to(DEV), ops.new_act(B, H, W, 8, DEV)
    ops.softmax_loss(lg, yd, probs, loss0, dl0, HW=H * W, C_classes=C, inv_global_batch=INV, quad_w=W if quad else 0)
    loss1 = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.loss_from_probs(probs, yd, loss1, HW=H * W, C_classes=C, inv_global_batch=INV)
    acc, dl1 = _launch(probs, yd, q.to(DEV), _table((2.0, 0.0, 1.0)), quad, C, B, H, W)
    print(f"\n  no soft weight: {acc[0].item():.7f} vs the CCE launch {loss0[0].item():.7f}, loss_from_probs {loss1[0].item():.7f}", end="")
    assert abs(acc[0].item() - loss0[0].item()) <= 1e-5 * abs(loss0[0].item())
    assert abs(acc[0].item() - loss1[0].item()) <= 1e-5 * abs(loss1[0].item())
    assert acc[5].item() == 0.0
    d0 = OL._from_quad(dl0.float())[..., :C] if quad else dl0.float()[..., :C]
    d1 = _classes(dl1, quad, C)
    p = probs.double().cpu()
    S = D.hard_G(p, y).abs() * INV
    mag = p * (S + (S * p).sum(-1, keepdim=True))
    assert_elementwise(d1.double().cpu(), d0.double().cpu(), mag, U_BF16, 4.0, tiny=2.0 ** -20 * INV, what="no soft weight")


def test_no_pixels_give_a_zero_loss_and_no_launch():
    """M = 0 through the C ABI (an empty tensor has no data pointer to pass): loss 0, the ticket at zero."""
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    acc = torch.zeros(ops.DISTILL_ACC_FLOATS, device=DEV)
    acc[0], acc[40] = 7.0, 5.0
    buf = torch.zeros(16, device=DEV)
    d = L.DistillDesc(0, 16, 3, 8, 0, 0.1, 1e-7, 0.25)
    L.check(L.load().usseg_distill_loss(ctypes.byref(d), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), _table(SETTINGS[0]).data_ptr(), acc.data_ptr(),
                                        acc.numel(), None, torch.cuda.current_stream().cuda_stream), "distill_loss")
    torch.cuda.synchronize()
    assert acc[0].item() == 0.0 and acc[1].item() == 0.0 and acc[40].item() == 5.0          # the header alone was set: no workgroup published a partial


def test_settings_changed_on_the_device_change_the_next_call_and_nothing_else():
    C, B, H, W = 3, 1, 64, 46
    p32, y, q, pd, yd, qd = _inputs(C, B, H, W)
    keep = [t.clone() for t in (pd, yd, qd)]
    table = _table(SETTINGS[0])
    acc1, dl1 = _launch(pd, yd, qd, table, True, C, B, H, W)
    first = (acc1[:6].clone(), dl1.clone())
    table.copy_(_table(SETTINGS[2]))                              # the SAME device table, new values
    acc2, dl2 = _launch(pd, yd, qd, table, True, C, B, H, W, acc=acc1)
    fresh_acc, fresh_dl = _launch(pd, yd, qd, _table(SETTINGS[2]), True, C, B, H, W)
    assert torch.equal(acc2[:6], fresh_acc[:6]) and torch.equal(dl2.view(torch.int16), fresh_dl.view(torch.int16))
    assert not torch.equal(first[0], acc2[:6]) and not torch.equal(first[1].view(torch.int16), dl2.view(torch.int16))
    assert first[0][2].item() == acc2[2].item()                   # the hard pixel sum does not depend on the settings
    assert all(torch.equal(a, b) for a, b in zip(keep, (pd, yd, qd)))
    _check("changed settings", acc2, dl2, True, C, p32, y, q, SETTINGS[2])


# ------------------------------------------------------------------------------------------------ the model
def _teacher(make, seed):
    """The same builder at another seed (the TransUNet builder of test_gpu_overlap_loss has its seed fixed: built here)."""
    import test_gpu_overlap_loss as OL
    import usseg_oracle as O
    if make == "archB":
        return OL._arch_b(seed=seed)
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True, use_vit=True, transunet=True).items()}
    net = VisionTransformer(img_size=(64, 64), batch_size=2, in_channels=1)
    net.load_params(P)
    return net


def _student(make, teacher, **kw):
    import test_gpu_overlap_loss as OL
    return (OL._arch_b if make == "archB" else OL._transunet)(loss="distill", teacher=teacher, **kw)


def _batches(n):
    import test_gpu_overlap_loss as OL
    return OL._batches(n, 2, 64, 64)


def _full_state(m):
    torch.cuda.synchronize()
    d = {f"p:{k}": v.clone() for k, v in m.export_params().items()}
    d.update({f"s:{i}": t.clone() for i, t in enumerate(m._graph_state())})
    return d


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("make", ["archB", "transunet"])
def test_the_model_steps_with_the_distillation_loss_and_the_teacher_stays_as_it_is(make):
    teacher = _teacher(make, 5)
    net = _student(make, teacher)
    assert net.distill_settings == {"temperature": 2.0, "soft_weight": 0.5, "hard_weight": 0.5} and net.loss_name == "distill"
    before = _full_state(teacher)
    x, y = _batches(1)[0]
    l, probs = net.step(x, y.float())
    q = teacher.predict(x).clone()
    torch.cuda.synchronize()
    inv = 1.0 / (2 * 64 * 64) if net.transunet else 0.5
    want, hard, soft = D.loss(probs.double().cpu(), y.double(), q.cpu(), 2.0, 0.5, 0.5, inv)
    print(f"\n  {make}: step loss {l.item():.6f}, restatement on its and the teacher's probabilities {want.item():.6f}", end="")
    assert math.isfinite(l.item()) and abs(l.item() - want.item()) <= 2e-5 * abs(want.item())
    terms = net.distill_terms()
    assert abs(terms["hard"] - inv * 0.5 * hard.item()) <= 2e-5 * inv * 0.5 * hard.item() and terms["soft"] > 0
    assert abs(terms["soft"] - inv * 0.5 * soft.item()) <= 2e-5 * abs(want.item())
    got = net.compute_loss(y.float(), probs)                        # no teacher in its arguments: the hard term, weighted
    if not net.transunet:
        assert got.shape == () and abs(got.item() - terms["hard"]) <= 2e-5 * terms["hard"]
    losses = []
    for _ in range(8):
        l, _p = net.train_step(x, y.float())
        losses.append(l.item())
    print(f"; {losses[0]:.4f} -> {losses[-1]:.4f}", end="")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert net._loss[1].item() == 0
    assert _same(before, _full_state(teacher)), "student steps changed the teacher"
    assert len(net.export_params()) == len(teacher.export_params())                                          # the teacher is no part of the student's variables


def test_an_ensemble_teacher_equals_feeding_its_probabilities_to_the_launch():
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.ensemble import Ensemble
    t1, t2 = _teacher("archB", 5), _teacher("archB", 6)
    ens = Ensemble([t1, t2], flip=True)
    net = _student("archB", ens, distill=dict(temperature=4.0, soft_weight=0.7, hard_weight=0.3))
    before = [_full_state(t1), _full_state(t2)]
    x, y = _batches(1)[0]
    l, probs = net.step(x, y.float())
    l, probs = l.clone(), probs.clone()
    q = ens.predict(x).probs.clone()
    acc = torch.zeros(ops.DISTILL_ACC_FLOATS, device=DEV)
    ops.distill_loss(probs, y.float().to(DEV), q, _table((4.0, 0.7, 0.3)), acc, None, HW=64 * 64, C_classes=3, inv_global_batch=0.5)
    torch.cuda.synchronize()
    assert acc[0].item() == l.item() and torch.equal(acc[:6], net._loss[:6])
    net.train_step(x, y.float())
    assert _same(before[0], _full_state(t1)) and _same(before[1], _full_state(t2))


@pytest.mark.parametrize("make", ["archB", "transunet"])
def test_graph_replay_equals_eager_and_follows_the_settings(make):
    from test_gpu_step import _assert_same_state, _state
    teachers = [_teacher(make, 5) for _ in range(3)]
    eager, graph = _student(make, teachers[0]), _student(make, teachers[1])
    tstate = _full_state(teachers[1])
    bs = _batches(5)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    _assert_same_state(_state(eager), _state(graph), "capture must not change the training state")
    assert _same(tstate, _full_state(teachers[1])), "capture changed the teacher"
    for i, (x, y) in enumerate(bs[:3]):
        l0, p0 = eager.train_step(x, y.float())
        l1, p1 = graph.train_step(x, y.float())
        torch.cuda.synchronize()
        assert l0.item() == l1.item(), (i, l0.item(), l1.item())
        assert torch.equal(p0, p1), i
        _assert_same_state(_state(eager), _state(graph), f"{make} step {i}")
    assert _same(tstate, _full_state(teachers[1])), "replays changed the teacher"
    # the SAME captured graph after set_distill(temperature=4) against an eager model BUILT with temperature 4 and brought to the same state
    hot = _student(make, teachers[2], distill=dict(temperature=4.0))
    hot.set_distill(temperature=2.0)
    for x, y in bs[:3]:
        hot.train_step(x, y.float())
    hot.set_distill(temperature=4.0)
    _assert_same_state(_state(hot), _state(graph), "the third model reached the same state")
    captured = graph._graph
    graph.set_distill(temperature=4.0)
    assert graph.distill_settings == hot.distill_settings == {"temperature": 4.0, "soft_weight": 0.5, "hard_weight": 0.5}
    seen = []
    for i, (x, y) in enumerate(bs[3:]):
        l0, p0 = hot.train_step(x, y.float())
        l1, p1 = graph.train_step(x, y.float())
        torch.cuda.synchronize()
        assert l0.item() == l1.item() and torch.equal(p0, p1), i
        _assert_same_state(_state(hot), _state(graph), f"{make} temperature 4 step {i}")
        seen.append(l1.item())
    assert graph._graph is captured and captured is not None
    la, _ = eager.train_step(bs[3][0], bs[3][1].float())              # the same weights and batch under temperature 2
    assert la.item() != seen[0]


def test_the_default_loss_does_not_move_and_save_load_keep_the_settings(tmp_path):
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.distill import Distill
    import test_gpu_overlap_loss as OL
    a = OL._arch_b(loss="cce")
    d = _student("archB", _teacher("archB", 5))
    bs = _batches(2)
    d.train_step(bs[0][0], bs[0][1].float())
    b = OL._arch_b()
    assert not isinstance(a._seg_loss, Distill) and not isinstance(b._seg_loss, Distill) and b.distill_settings is None and b.distill_terms() is None
    assert a._loss.numel() == b._loss.numel() == ops.ACC_FLOATS
    with pytest.raises(ValueError):
        b.set_distill(temperature=2.0)
    for x, y in bs:
        la, pa = a.train_step(x, y.float())
        lb, pb = b.train_step(x, y.float())
        torch.cuda.synchronize()
        assert la.item() == lb.item() and torch.equal(pa, pb)
    assert torch.equal(a.flat.flat, b.flat.flat)
    assert not torch.equal(a.flat.flat, d.flat.flat)
    # save / load
    d.set_distill(temperature=3.0, soft_weight=0.25)
    assert d.distill_settings == {"temperature": 3.0, "soft_weight": 0.25, "hard_weight": 0.5}
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(temperature=9.0), dict(soft_weight=-1.0), dict(soft_weight=0.0, hard_weight=0.0)):
        with pytest.raises(ValueError):
            d.set_distill(**bad)
    assert d.distill_settings == {"temperature": 3.0, "soft_weight": 0.25, "hard_weight": 0.5}        # a refused call changes nothing
    d.save(str(tmp_path / "m.pt"))
    e = _student("archB", _teacher("archB", 6))
    assert e.distill_settings["temperature"] == 2.0
    e.load(str(tmp_path / "m.pt"))
    assert e.distill_settings == d.distill_settings and torch.equal(e.flat.flat, d.flat.flat)
    b.load(str(tmp_path / "m.pt"))                                    # a model without the loss ignores the entry
    assert torch.equal(b.flat.flat, d.flat.flat)


def test_the_refusals():
    import test_gpu_overlap_loss as OL
    from ultrasound_modeling_amd.distill import Distill
    from ultrasound_modeling_amd.ensemble import Ensemble
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    t = _teacher("archB", 5)
    kw = dict(batch_size=2, img_size=(64, 64), in_channels=1)
    with pytest.raises(ValueError, match="needs teacher="):
        VisionTransformer(loss="distill", **kw)
    with pytest.raises(ValueError, match="only apply to loss in"):
        VisionTransformer(loss="cce", teacher=t, **kw)
    with pytest.raises(ValueError, match="only apply to loss in"):
        VisionTransformer(loss="dice", overlap={}, distill={}, **kw)
    for other in (dict(class_factor=[1, 1, 1]), dict(focal_gamma=2), dict(overlap={}), dict(boundary={}), dict(lovasz={}), dict(topk={})):
        with pytest.raises(ValueError, match="do not combine"):
            VisionTransformer(loss="distill", teacher=t, **other, **kw)
    with pytest.raises(ValueError, match="VisionTransformer .* or an Ensemble"):
        VisionTransformer(loss="distill", teacher=object(), **kw)
    with pytest.raises(ValueError, match="image size"):
        VisionTransformer(loss="distill", teacher=t, batch_size=2, img_size=(64, 80), in_channels=1)
    with pytest.raises(ValueError, match="input channels"):
        VisionTransformer(loss="distill", teacher=t, batch_size=2, img_size=(64, 64), in_channels=2)
    with pytest.raises(ValueError, match="class count"):
        VisionTransformer(loss="distill", teacher=t, num_classes=2, **kw)
    s = _student("archB", t)
    with pytest.raises(ValueError, match="the student itself"):
        Distill(s, None, s)
    with pytest.raises(ValueError, match="the student itself"):
        Distill(Ensemble([t, s]), None, s)

    class _Dropout(Ensemble):                                          # what an Ensemble of Arch A members reports: a dropout counter its predict advances
        def _predict_state(self):
            return [torch.zeros(1, device=DEV)]
    with pytest.raises(ValueError, match="advances device state"):
        Distill(_Dropout([t]), None, s)


# ------------------------------------------------------------------------------------------------ two ranks
TWO_RANK_DISTILL = dict(temperature=2.0, soft_weight=0.5, hard_weight=0.5)
TEACHER_SEED = 9


def test_two_gloo_ranks_with_the_distillation_loss_equal_the_simulation_bit_for_bit(tmp_path):
    """tests/test_gpu_topk.py's two-rank test with ``main(..., loss="distill", teacher=...)``: nine images in batches of four, so the last step
    leaves rank 1 without an image; every replica's teacher sees its slice; ranks and simulation each in a fresh process."""
    import test_gpu_mainparallel as MP
    train, val = MP._arrays(MP.N_TRAIN, seed=1), MP._arrays(MP.N_TEST, seed=2)
    np.save(tmp_path / "train.npy", train)
    np.save(tmp_path / "val.npy", val)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "USSEG_DP_CHUNKS")}
    env.update(USSEG_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc_per_node", "2", "--master_addr", "127.0.0.1",
                        "--master_port", str(MP._free_port()), os.path.abspath(__file__), str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "distill terms: hard = " in r.stdout                                       # the drivers' extra report line
    d = [torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2)]
    assert d[0]["graph"] and d[1]["graph"] and d[0]["loss_name"] == "distill"
    assert torch.equal(d[0]["state"]["flat"], d[1]["state"]["flat"]), "replicas diverged"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path), "simulate"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    sim = torch.load(tmp_path / "sim.pt", weights_only=False)
    want, history = sim["want"], sim["history"]
    for k in range(2):
        assert MP._first_difference(d[k]["state"], want[k]) is None, (k, MP._first_difference(d[k]["state"], want[k]))
    assert want[0]["step"].item() == MP.EPOCHS * 3                                     # three steps an epoch: the last one with an empty rank 1
    MP._same_history(d[0]["history"], history)
    MP._same_history(d[1]["history"], history)


def _two_rank_teacher():
    """A teacher every process builds alike (the constructor's seeded initialisation), on the device ``main`` puts the student on."""
    import test_gpu_mainparallel as MP
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    return VisionTransformer(2, img_size=(MP.H, MP.W), in_channels=MP.C, use_vit=False, seed=TEACHER_SEED, device=MP.DEV)


def _rank(tmp):
    import torch.distributed as dist
    import test_gpu_mainparallel as MP
    from ultrasound_modeling_amd.MainParallel import main
    teacher = _two_rank_teacher()
    net, proc = main(os.path.join(tmp, "train.npy"), os.path.join(tmp, "val.npy"), None, epochs=MP.EPOCHS, batch_size=MP.B, use_vit=False,
                     seed=MP.SEED, loss="distill", teacher=teacher, distill=TWO_RANK_DISTILL)
    rank = dist.get_rank()
    torch.save({"state": MP._state(net), "history": proc.history, "graph": net._graph is not None, "loss_name": net.loss_name},
               os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _simulate(tmp):
    """``test_gpu_mainparallel._simulate`` with both instances built with ``loss="distill"`` and a teacher of their own."""
    import test_gpu_mainparallel as MP
    import ultrasound_modeling_amd.VisionTransformer as VT
    from ultrasound_modeling_amd.distill import Distill
    orig, made = VT.VisionTransformer, []

    def make(*a, **kw):
        VT.VisionTransformer = orig               # (the class itself while the teacher and the student are built: the owner checks isinstance)
        try:
            made.append(orig(*a, loss="distill", teacher=_two_rank_teacher(), distill=TWO_RANK_DISTILL, **kw))
        finally:
            VT.VisionTransformer = make
        return made[-1]
    VT.VisionTransformer = make
    want, history = MP._simulate(np.load(os.path.join(tmp, "train.npy")), np.load(os.path.join(tmp, "val.npy")))
    assert len(made) == 2 and all(n.loss_name == "distill" and isinstance(n._seg_loss, Distill) for n in made), "the simulation did not train with distill"
    torch.save({"want": want, "history": history}, os.path.join(tmp, "sim.pt"))


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    if sys.argv[2:] == ["simulate"]:
        _simulate(sys.argv[1])
    else:
        _rank(sys.argv[1])
