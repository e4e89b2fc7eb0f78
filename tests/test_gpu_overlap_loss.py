"""The region-overlap losses (soft Dice / Tversky, optionally plus CCE; usseg.h UssegOverlapLoss, csrc/overlap_loss.hip) on the GPU:

  * pass 1 (``ops.overlap_loss_sums``): the totals I, P, Y per class against the fp64 restatement (tests/overlap_restatement.py), three calls
    bit for bit, the ticket back at zero, the scalar loss and the backward coefficients;
  * pass 2 (``ops.overlap_loss_bwd``): ``dlogits`` per element, row and quad layouts, C in {2, 3, 4}, pad channels exactly zero;
  * the CCE limit (``ov_weight = 0, ce_weight = 1``) against the existing loss_kind 0 launch;
  * Arch B at 64x64 and the TransUNet variant: every new ``loss=`` steps finitely, falls on a fixed batch, replays from a graph bit for bit;
    two gloo ranks equal the two-instance simulation bit for bit (an empty replica included); ``loss="cce"`` does not move.

Bounds.  Totals: every term p*y, p, y is non-negative, so a total summed in fp32 along chains of at most d roundings is within
gamma_d = d*u/(1 - d*u), u = 2^-24, RELATIVE of the exact sum; d comes from the grid rule usseg.h states (``R.sum_depth``: per-thread groups,
wave butterfly, workgroup tree, every-sixteenth-workgroup strands, strand tree, the product's rounding).  The fp64 restatement's own error
(2^-53 * M) is five orders below that.  Scalar loss: 1e-5 relative, the project's bar for a scalar loss (tests/test_gpu_class_loss.py).
dlogits: |dl - ref| <= 4 * 2^-8 * mag + tiny (route_probe's construction, as tests/test_gpu_class_loss.py uses it) with mag from the
restatement - the sizes of the terms |A_c|*|y_c| + |B_c| (+ the CCE term) carried through p_k*(G_k - sum_c G_c*p_c): one bf16 rounding (2^-9)
on top of fp32 arithmetic, and coefficients whose own relative error (3 totals, gamma_d each, plus a handful of roundings: < 2^-17) is far
inside 2^-8.  tiny = 2^-20 * ov_weight*ov_scale*max(w)*power / min_c D_c (+ 2^-20 * ce_weight*inv_global_batch with a CCE term): 2^-20
(route_probe's fp32 unit) of the gradient scale k_c/D_c of a pixel whose probabilities are O(1).  With a CCE term, a pixel whose fp64
probability lies within 2^-20 relative of a clip constant may be left out, at most 1e-3 of the pixels; the inputs (logits from N(0, 2^2))
have none (tests/test_cpu_overlap_loss.py), and without a CCE term no pixel is ever left out.
"""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import overlap_restatement as R
import usseg_oracle as O
from route_probe import assert_elementwise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
U_BF16 = 2.0 ** -8
NEW_LOSSES = ["dice", "tversky", "dice_ce"]
SHAPES = [(2, 256, 80), (1, 64, 47), (1, 9, 7)]          # 40 workgroups; 3 workgroups, the last one partly idle; 63 pixels: a partial last group


def _ol(cfg):
    from ultrasound_modeling_amd import ops
    return ops.overlap_loss(cfg["w"], cfg["alpha"], cfg["beta"], cfg["smooth"], cfg["power"], cfg["ov_weight"], cfg["ce_weight"])


def _cfg(loss, C, power=1.0):
    return R.config(loss, C, power=power, w=[(0.2 + 0.3 * c) / C for c in range(C)])


def _probs(logits):
    """fp32 probabilities as the head leaves them (any fp32 softmax will do: the restatement is then taken at THESE probabilities)."""
    return torch.softmax(logits.float(), -1).contiguous()


def _to_quad_shape(B, H, W):
    return (B, H // 2, W // 2, 16)


def _from_quad(q):
    B, h, w, _ = q.shape
    out = torch.zeros(B, 2 * h, 2 * w, 4, dtype=q.dtype, device=q.device)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + 4]
    return out


def _restate_at(p32, y, cfg, inv, ov_scale):
    """The restatement's loss, totals, coefficients and gradient at GIVEN fp32 probabilities (fp64 arithmetic)."""
    p = p32.double().cpu().clone().requires_grad_(True)
    l = R.loss(p, y, cfg, inv, ov_scale)
    l.backward()
    I, P, Y = R.sums(p.detach(), y)
    _, D, T = R.tversky(I, P, Y, cfg["alpha"], cfg["beta"], cfg["smooth"])
    A, Bc = R.coefficients(I, P, Y, cfg, ov_scale)
    return dict(loss=l.item(), I=I, P=P, Y=Y, T=T, D=D, A=A, B=Bc, G=p.grad)


# ------------------------------------------------------------------------------------------------ pass 1
# every small shape with and without the CCE sum; then 136 workgroups (two rounds of strand loads) and 552960 pixels (the 512-workgroup cap: two
# groups a thread, 32 workgroups a strand) once each
SUM_CASES = [(loss, C) + shp for loss in ("tversky", "dice_ce") for C in (3, 2, 4) for shp in SHAPES] + [("dice_ce", 3, 2, 256, 272), ("dice_ce", 3, 1, 768, 720)]


@pytest.mark.parametrize("loss,C,B,H,W", SUM_CASES)
def test_sums_against_the_restatement_and_bit_for_bit_over_three_calls(loss, C, B, H, W):
    from ultrasound_modeling_amd import ops
    M = B * H * W
    logits, y = R.inputs(C, B, H, W)
    cfg = _cfg(loss, C, power=2.0)
    inv, ov_scale = 1.0 / 7.0, 0.5
    p32 = _probs(logits)
    want = _restate_at(p32, y, cfg, inv, ov_scale)
    pd, yd = p32.to(DEV), y.float().to(DEV)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    runs = []
    for _ in range(3):
        ops.overlap_loss_sums(pd, yd, acc, overlap=_ol(cfg), HW=H * W, C_classes=C, ov_scale=ov_scale, inv_global_batch=inv)
        torch.cuda.synchronize()
        runs.append(acc[:32].cpu().clone())
        assert acc[1].item() == 0                              # the ticket counter is back at zero: no per-call zeroing
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    got = runs[0].double()
    bound = R.sum_bound(M)
    depth, grid = R.sum_depth(M)
    assert ops.overlap_loss_grid(M) == grid
    for name, off in (("I", 16), ("P", 20), ("Y", 24)):
        err = ((got[off:off + C] - want[name]).abs() / want[name]).max().item()
        print(f"\n  {loss} C={C} {B}x{H}x{W} grid {grid} depth {depth}: {name} rel err {err:.2e} (bound {bound:.2e})", end="")
        assert err <= bound
    # T and the coefficients: three totals (gamma_d each) and fewer than 16 further roundings; (1 - T)^(g-1) amplifies T's error by (g-1)*T/(1-T)
    amp = 1.0 + (cfg["power"] - 1.0) * (want["T"] / (1.0 - want["T"])).max().item()
    cb = (3 * bound + 16 * 2.0 ** -24) * amp
    assert ((got[28:28 + C] - want["T"]).abs() <= cb * want["T"]).all()
    assert ((got[4:4 + C] - want["A"]).abs() <= cb * want["A"].abs()).all()
    assert ((got[8:8 + C] - want["B"]).abs() <= cb * want["B"].abs()).all()
    print(f"\n  loss {got[0].item():.7f} vs {want['loss']:.7f}", end="")
    assert abs(got[0].item() - want["loss"]) <= 1e-5 * abs(want["loss"])


def test_sums_of_no_pixels_give_a_zero_loss():
    """M = 0 through the C ABI (an empty tensor has no data pointer to pass): loss 0, the ticket at zero."""
    import ctypes as C
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    acc[0] = 7.0
    buf = torch.zeros(16, device=DEV)
    d = L.LossDesc(0, 16, 3, 3, 8, 0, 0.1, 1e-7, 0.25, 0)
    ol = _ol(_cfg("dice_ce", 3))
    L.check(L.load().usseg_overlap_loss_sums(C.byref(d), C.byref(ol), 0.0, buf.data_ptr(), buf.data_ptr(), acc.data_ptr(), acc.numel(),
                                             torch.cuda.current_stream().cuda_stream), "overlap_loss_sums")
    torch.cuda.synchronize()
    assert acc[0].item() == 0.0 and acc[1].item() == 0.0


# ------------------------------------------------------------------------------------------------ pass 2
def _run_both(loss, C, B, H, W, quad, power=1.0, inv=0.25, ov_scale=0.5, cfg=None):
    from ultrasound_modeling_amd import ops
    logits, y = R.inputs(C, B, H, W)
    cfg = cfg or _cfg(loss, C, power)
    p32 = _probs(logits)
    pd, yd = p32.to(DEV), y.float().to(DEV)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    kw = dict(overlap=_ol(cfg), HW=H * W, C_classes=C, inv_global_batch=inv)
    ops.overlap_loss_sums(pd, yd, acc, ov_scale=ov_scale, **kw)
    dl = torch.full(_to_quad_shape(B, H, W) if quad else (B, H, W, 8), float("nan"), dtype=torch.bfloat16, device=DEV)   # every element must be written
    ops.overlap_loss_bwd(pd, yd, acc, dl, quad_w=W if quad else 0, **kw)
    torch.cuda.synchronize()
    return cfg, p32, y, acc, dl


def _check_dlogits(what, d, p32, y, cfg, inv, ov_scale):
    """d [B,H,W,C] against the restatement taken at the same fp32 probabilities."""
    p = p32.double()
    want = _restate_at(p32, y, cfg, inv, ov_scale)
    G = want["G"]
    ref = p * (G - (G * p).sum(-1, keepdim=True))
    S = want["A"].abs() * y.abs() + want["B"].abs()
    tiny = 2.0 ** -20 * cfg["ov_weight"] * ov_scale * max(cfg["w"]) * cfg["power"] / want["D"].min().item()
    skip = torch.zeros(p.shape[:-1], dtype=torch.bool)
    if cfg["ce_weight"] != 0.0:
        pc = p.clone().requires_grad_(True)
        (cfg["ce_weight"] * inv * R.cce_per_pixel(pc, y).sum()).backward()
        S = S + pc.grad.abs()
        tiny += 2.0 ** -20 * cfg["ce_weight"] * inv
        q = p / p.sum(-1, keepdim=True)
        rel = 2.0 ** -20
        skip = (((q - R.LO).abs() <= rel * R.LO) | ((q - R.HI).abs() <= rel * R.HI)).any(-1)
    mag = p * (S + (S * p).sum(-1, keepdim=True))
    n_skip = int(skip.sum())
    print(f"\n  {what}: {n_skip} of {skip.numel()} pixels at a clip edge left out", end="")
    assert n_skip <= (1e-3 * skip.numel() if cfg["ce_weight"] != 0.0 else 0)
    keep = ~skip
    assert_elementwise(d.double().cpu()[keep], ref[keep], mag[keep], U_BF16, 4.0, tiny=tiny, what=what)


@pytest.mark.parametrize("loss,power", [("dice", 1.0), ("tversky", 2.0), ("dice_ce", 1.0), ("dice_ce", 2.0)])
@pytest.mark.parametrize("C", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_dlogits_row_layout_per_element(loss, power, C, B, H, W):
    cfg, p32, y, acc, dl = _run_both(loss, C, B, H, W, quad=False, power=power)
    assert dl[..., C:].float().abs().max().item() == 0                # pad channels exactly zero (and written: the buffer started as NaN)
    _check_dlogits(f"row {loss} g={power} C={C} {B}x{H}x{W}", dl[..., :C].float(), p32, y, cfg, 0.25, 0.5)


@pytest.mark.parametrize("loss,power", [("tversky", 1.0), ("dice_ce", 2.0)])
@pytest.mark.parametrize("C", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", [(2, 256, 80), (1, 64, 46), (3, 10, 6)])      # (the quad layout needs even H and W: 64x46 stands in for 64x47)
def test_dlogits_quad_layout_per_element(loss, power, C, B, H, W):
    cfg, p32, y, acc, dl = _run_both(loss, C, B, H, W, quad=True, power=power)
    d4 = _from_quad(dl.float())
    assert not torch.isnan(d4).any()                                  # all 16 channels of every quad pixel were written
    if C < 4:
        assert d4[..., C:].abs().max().item() == 0                    # the pad classes of every parity slot
    _check_dlogits(f"quad {loss} g={power} C={C} {B}x{H}x{W}", d4[..., :C], p32, y, cfg, 0.25, 0.5)


@pytest.mark.parametrize("quad", [False, True])
def test_the_cce_limit_equals_the_existing_cce_launch(quad):
    """ov_weight = 0, ce_weight = 1: the loss and dlogits of the existing loss_kind 0 launch on the same logits, dlogits with the per-element bound."""
    from ultrasound_modeling_amd import ops
    C, B, H, W, inv = 3, 2, 64, 46, 0.25
    logits, y = R.inputs(C, B, H, W)
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
    ops.softmax_loss(lg, yd, probs, loss0, dl0, HW=H * W, C_classes=C, inv_global_batch=inv, quad_w=W if quad else 0)
    cfg = R.config("dice_ce", C, ov_weight=0.0, ce_weight=1.0)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    kw = dict(overlap=_ol(cfg), HW=H * W, C_classes=C, inv_global_batch=inv)
    ops.overlap_loss_sums(probs, yd, acc, ov_scale=1.0, **kw)
    dl1 = torch.full_like(dl0, float("nan"))
    ops.overlap_loss_bwd(probs, yd, acc, dl1, quad_w=W if quad else 0, **kw)
    torch.cuda.synchronize()
    print(f"\n  CCE limit: {acc[0].item():.7f} vs the CCE launch {loss0[0].item():.7f}", end="")
    assert abs(acc[0].item() - loss0[0].item()) <= 1e-5 * abs(loss0[0].item())
    d0, d1 = (_from_quad(dl0.float())[..., :C], _from_quad(dl1.float())[..., :C]) if quad else (dl0.float()[..., :C], dl1.float()[..., :C])
    p = probs.double().cpu()
    pc = p.clone().requires_grad_(True)
    (inv * R.cce_per_pixel(pc, y).sum()).backward()
    S = pc.grad.abs()
    mag = p * (S + (S * p).sum(-1, keepdim=True))
    assert_elementwise(d1.double().cpu(), d0.double().cpu(), mag, U_BF16, 4.0, tiny=2.0 ** -20 * inv, what="CCE limit")
    _check_dlogits("CCE limit vs restatement", d1, probs.cpu(), y, cfg, inv, 1.0)


# ------------------------------------------------------------------------------------------------ the model
def _arch_b(seed=3, **kw):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True).items()}
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1, learning_rate=1e-3, **kw)
    net.load_params(P)
    return net


def _transunet(**kw):
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=21, perturb=True, use_vit=True, transunet=True).items()}
    net = VisionTransformer(img_size=(64, 64), batch_size=2, in_channels=1, **kw)
    net.load_params(P)
    return net


def _batches(n, B, H, W):
    return [tuple(t for t in O.synthetic_batch(B, H, W, 1, seed=40 + i)) for i in range(n)]


def _model_cfg(net):
    ol = net.overlap_loss
    return dict(w=list(ol.w)[:net.num_classes], alpha=ol.alpha, beta=ol.beta, smooth=ol.smooth, power=ol.power, ov_weight=ol.ov_weight, ce_weight=ol.ce_weight)


@pytest.mark.parametrize("loss", NEW_LOSSES)
@pytest.mark.parametrize("make", [_arch_b, _transunet], ids=["archB", "transunet"])
def test_the_model_steps_with_the_overlap_loss_and_the_loss_falls(make, loss):
    net = make(loss=loss, overlap=dict(power=2.0) if loss == "tversky" else {})
    x, y = _batches(1, 2, 64, 64)[0]
    l, probs = net.step(x, y.float())
    torch.cuda.synchronize()
    # the step's loss is the restatement at its own probabilities: Arch B divides the CCE by the global batch, the TransUNet variant by B*H*W
    inv = 1.0 / (2 * 64 * 64) if net.transunet else 0.5
    want = R.loss(probs.double().cpu(), y, _model_cfg(net), inv, 1.0).item()
    print(f"\n  {loss}: step loss {l.item():.6f}, restatement on its probabilities {want:.6f}", end="")
    assert math.isfinite(l.item()) and abs(l.item() - want) <= 2e-5 * abs(want)
    got = net.compute_loss(y.float(), probs)
    if not net.transunet:                                            # compute_loss divides by the global batch, as it does for every loss
        assert got.shape == () and abs(got.item() - want) <= 2e-5 * abs(want)
    losses = []
    for _ in range(8):
        l, _p = net.train_step(x, y.float())
        losses.append(l.item())
    print(f"; {losses[0]:.4f} -> {losses[-1]:.4f}", end="")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert net._loss[1].item() == 0


@pytest.mark.parametrize("loss", NEW_LOSSES)
@pytest.mark.parametrize("make", [_arch_b, _transunet], ids=["archB", "transunet"])
def test_graph_replay_equals_eager_with_the_overlap_loss(make, loss):
    from test_gpu_step import _assert_same_state, _state
    eager, graph = make(loss=loss, overlap={}), make(loss=loss, overlap={})
    bs = _batches(3, 2, 64, 64)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    _assert_same_state(_state(eager), _state(graph), "capture must not change the training state")
    for i, (x, y) in enumerate(bs):
        l0, p0 = eager.train_step(x, y.float())
        l1, p1 = graph.train_step(x, y.float())
        torch.cuda.synchronize()
        assert l0.item() == l1.item(), (i, l0.item(), l1.item())
        assert torch.equal(p0, p1), i
        _assert_same_state(_state(eager), _state(graph), f"{loss} step {i}")
    assert _state(graph)["step"] == 3
    # a short batch after the capture runs eagerly, through the same two passes
    x, y = _batches(1, 1, 64, 64)[0]
    l0, _ = eager.train_step(x, y.float())
    l1, _ = graph.train_step(x, y.float())
    assert l0.item() == l1.item()


def test_the_default_loss_does_not_move_across_the_new_code():
    """loss="cce" built before and after a Dice model has been built and stepped: the same bits, and not one overlap buffer."""
    a = _arch_b(loss="cce")
    d = _arch_b(loss="dice", overlap={})
    bs = _batches(2, 2, 64, 64)
    d.train_step(bs[0][0], bs[0][1].float())
    b = _arch_b()
    from ultrasound_modeling_amd import ops
    assert a.overlap_loss is None and b.overlap_loss is None and a._loss.numel() == b._loss.numel() == ops.ACC_FLOATS
    for x, y in bs:
        la, pa = a.train_step(x, y.float())
        lb, pb = b.train_step(x, y.float())
        torch.cuda.synchronize()
        assert la.item() == lb.item() and torch.equal(pa, pb)
    assert torch.equal(a.flat.flat, b.flat.flat)
    assert not torch.equal(a.flat.flat, d.flat.flat)


def test_the_bare_name_is_refused_and_the_empty_dict_takes_the_defaults():
    """``loss="dice"`` alone stays the ValueError it was before these losses existed; ``overlap={}`` selects the defaults."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for loss in NEW_LOSSES:
        with pytest.raises(ValueError):
            VisionTransformer(2, (64, 64), in_channels=1, loss=loss)
    net = VisionTransformer(2, (64, 64), in_channels=1, loss="tversky", overlap={})
    c = _model_cfg(net)
    assert (round(c["alpha"], 6), round(c["beta"], 6), c["smooth"], c["power"], c["ov_weight"], c["ce_weight"]) == (0.3, 0.7, 1.0, 1.0, 1.0, 0.0)


def test_keywords_and_the_dict_reach_the_kernel_alike():
    a = _arch_b(loss="tversky", overlap=dict(alpha=0.6, beta=0.4, smooth=2.0, class_weight=[0.2, 0.3, 0.5]))
    b = _arch_b(loss="tversky", alpha=0.6, beta=0.4, smooth=2.0, class_weight=[0.2, 0.3, 0.5])
    x, y = _batches(1, 2, 64, 64)[0]
    la, pa = a.step(x, y.float())
    lb, _ = b.step(x, y.float())
    want = R.loss(pa.double().cpu(), y, _model_cfg(a), 0.5, 1.0).item()
    assert la.item() == lb.item() and abs(la.item() - want) <= 2e-5 * abs(want)
    assert _model_cfg(a)["alpha"] == pytest.approx(0.6) and _model_cfg(a)["smooth"] == 2.0


# ------------------------------------------------------------------------------------------------ the drivers' validation report
class _StubNet:
    """What the drivers' ``test`` use of a model: ``device``, ``step`` and the public ``overlap_loss`` property."""

    def __init__(self, overlap):
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.overlap_loss = overlap
        g = torch.Generator().manual_seed(9)
        self.probs = torch.softmax(2 * torch.randn(4, 16, 16, 3, generator=g), -1).to(self.device)

    def step(self, x, y, train=False):
        return torch.ones((), device=self.device), self.probs


class _StubData:
    num_te = 4

    def __init__(self, dev):
        g = torch.Generator().manual_seed(10)
        self.x = torch.zeros(4, 16, 16, 1, device=dev)
        self.y = torch.nn.functional.one_hot(torch.randint(0, 3, (4, 16, 16), generator=g), 3).float().to(dev)

    def next_test(self, n):
        return self.x, self.y, True

    def test_batches(self, rank, world):
        yield self.x, self.y, 4


def _report_labels(out):
    lines = out[out.index("Test..."):].splitlines()[1:]
    return [l.split(" = ")[0] for l in lines if " = " in l]


@pytest.mark.parametrize("with_overlap", [False, True])
def test_the_three_drivers_print_the_same_report_and_the_dice_line_only_with_an_overlap_loss(with_overlap, capsys):
    """loss, IoU, f1, precision, recall - the reference's five lines, in its order, from every driver and for every loss - and then the
    per-class Dice list exactly when the model trains with an overlap loss."""
    import types
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    from ultrasound_modeling_amd.metrics import SegMetrics, dice_per_class
    net = _StubNet(_ol(_cfg("dice", 3)) if with_overlap else None)
    data = _StubData(net.device)
    want = ["loss", "IoU", "f1", "precision", "recall"] + (["dice per class"] if with_overlap else [])
    ref = SegMetrics(3, round=True, device=net.device)
    ref.update_state(data.y, net.probs)
    dice = str(dice_per_class(ref.counts.cpu()))
    outs = {}
    MainNumpy.Process(batch_size=4, device=net.device).test(net, data, 0)
    outs["MainNumpy"] = capsys.readouterr().out
    TBI_TransUNet.test(net, data, 0)
    outs["TBI_TransUNet"] = capsys.readouterr().out
    proc = MainParallel.Process(4, capture_graph=False)
    proc.trainer = types.SimpleNamespace(net=net, rank=0, world=1)         # (what ``_mirror`` sets up around a real model)
    proc.metrics, proc.tr_metrics = SegMetrics(3, round=True, device=net.device), SegMetrics(3, round=True, device=net.device)
    proc._zero = torch.zeros((), device=net.device)
    proc.test(net, data, 0)
    outs["MainParallel"] = capsys.readouterr().out
    for name, out in outs.items():
        assert _report_labels(out) == want, (name, out)
        assert (("dice per class = " + dice) in out) == with_overlap, (name, out)
    assert "dice" not in proc.history[-1] and "dice" not in TBI_TransUNet.history[-1]      # the histories keep their keys


# ------------------------------------------------------------------------------------------------ two ranks
def test_two_gloo_ranks_with_dice_ce_equal_the_simulation_bit_for_bit(tmp_path):
    """tests/test_gpu_mainparallel.py's world of two (gloo, both ranks on device 0; nine images in batches of four, so the last step leaves
    rank 1 without an image) with ``main(..., loss="dice_ce")`` against its two-instance eager simulation built with the same loss.
    The simulation runs in a fresh process of its own, like the ranks: what a long pytest process has run before (workspaces grown by larger
    models, tests/test_gpu_model.py for one) changes the split of some weight-gradient sums and so the last bits of an in-process simulation -
    of every loss, the default included - which is not what this test is about."""
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
    assert "dice per class = [" in r.stdout                                           # the drivers' extra report line
    d = [torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2)]
    assert d[0]["graph"] and d[1]["graph"] and d[0]["loss_name"] == "dice_ce"
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


def _rank(tmp):
    import torch.distributed as dist
    import test_gpu_mainparallel as MP
    from ultrasound_modeling_amd.MainParallel import main
    net, proc = main(os.path.join(tmp, "train.npy"), os.path.join(tmp, "val.npy"), None, epochs=MP.EPOCHS, batch_size=MP.B, use_vit=False,
                     seed=MP.SEED, loss="dice_ce")
    rank = dist.get_rank()
    torch.save({"state": MP._state(net), "history": proc.history, "graph": net._graph is not None, "loss_name": net.loss_name},
               os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _simulate(tmp):
    """``test_gpu_mainparallel._simulate`` with both instances built with ``loss="dice_ce"``."""
    import test_gpu_mainparallel as MP
    import ultrasound_modeling_amd.VisionTransformer as V
    orig, made = V.VisionTransformer, []

    def make(*a, **kw):
        made.append(orig(*a, loss="dice_ce", overlap={}, **kw))
        return made[-1]
    V.VisionTransformer = make
    want, history = MP._simulate(np.load(os.path.join(tmp, "train.npy")), np.load(os.path.join(tmp, "val.npy")))
    assert len(made) == 2 and all(n.loss_name == "dice_ce" and n.overlap_loss is not None for n in made), "the simulation did not train with dice_ce"
    torch.save({"want": want, "history": history}, os.path.join(tmp, "sim.pt"))


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    if sys.argv[2:] == ["simulate"]:
        _simulate(sys.argv[1])
    else:
        _rank(sys.argv[1])
