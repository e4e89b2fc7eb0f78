"""The class loss (VisionTransformer.my_loss_cat and its focal variant; usseg.h UssegClassLoss, loss_kind 2) on the GPU:

  * every kernel that carries it - ``softmax_loss`` flat and quad, the fused head, ``loss_from_probs`` scalar and map - against the fp64
    restatement (tests/loss_restatement.py) for the three forms: my_loss_cat as committed, focal gamma 2, weighted focal gamma 1.5;
  * the fused head against its three launches, the uniform-weight class loss against the existing loss_kind 0 launch;
  * the default did not move; Arch B trains with every loss (step == restatement on its probabilities, graph replay == eager, the loss falls);
    the public ``my_loss_cat`` / ``compute_loss``; the TransUNet variant's per-pixel mean; the constructor's ValueErrors;
  * two gloo ranks with ``loss="my_loss_cat"`` equal the two-instance eager simulation bit for bit.

Bars (all the project's own): probabilities rel L2 < 1e-5, scalar 1e-5 relative, map rel L2 < 1e-5 (test_softmax_cce_loss_fwd_bwd,
test_my_loss_cat_on_probabilities).  dlogits per element, route_probe style: |dl - ref| <= 4 * 2^-8 * mag + tiny with
mag[k] = p[k]*(|dLdp[k]| + sum_c |dLdp[c]|*p[c]) from the restatement - the sizes of the terms of p[k]*(dLdp[k] - sum_c dLdp[c]*p[c]), one
bf16 rounding (2^-9) on top of fp32 arithmetic - and tiny = 2^-20 * factor * max(w) * inv_global_batch: 2^-20 (route_probe's fp32 unit) of the
gradient scale of a pixel whose probabilities are O(1).  Pad classes and pad slots are exactly zero.  A pixel with an fp64 probability within
2^-20 relative of a clip constant may be left out (fp32 may clip where fp64 does not): at most 0.1 % of the pixels, counted and printed.  The
forced row [40, -40, 0] is NOT left out: every class of it is clipped by orders of magnitude in either arithmetic, so its gradient is exactly 0.
"""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_restatement as R
import usseg_oracle as O
from route_probe import assert_elementwise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
REL_BF16 = 1e-3          # tests/test_gpu_ops.py
U_BF16 = 2.0 ** -8
FORM_NAMES = list(R.FORMS)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _cl(w, gamma, factor):
    from ultrasound_modeling_amd import ops
    return ops.class_loss(w, gamma, factor)


def _check_dlogits(what, dl, r, w, factor, inv, forced=None):
    """dl [..., C] (pads already checked) against the restatement r, per element."""
    tiny = 2.0 ** -20 * factor * max(w) * inv
    skip = r["edge"].clone()
    if forced is not None:
        assert r["dLdp"][forced].abs().max().item() == 0                   # clipped on every class in fp64 ...
        assert dl[forced].abs().max().item() == 0, dl[forced]              # ... and in the kernel: exactly no gradient
        skip[forced] = False
    n_skip, n_pix = int(skip.sum()), skip.numel()
    print(f"\n  {what}: {n_skip} of {n_pix} pixels at a clip edge left out", end="")
    assert n_skip <= 1e-3 * n_pix
    keep = ~skip
    assert_elementwise(dl.double().cpu()[keep], r["dlogits"][keep], r["mag"][keep], U_BF16, 4.0, tiny=tiny, what=what)


def _to_quad(l):
    """[B,H,W,C] -> the head's space-to-depth layout [B,H/2,W/2,16]: pixel (y,x) in slot 4*((y&1)*2+(x&1))."""
    B, H, W, C = l.shape
    q = torch.zeros(B, H // 2, W // 2, 16, dtype=l.dtype)
    for a in range(2):
        for b in range(2):
            q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + C] = l[:, a::2, b::2, :]
    return q


def _from_quad(q):
    """[B,h,w,16] -> [B,2h,2w,4]"""
    B, h, w, _ = q.shape
    out = torch.zeros(B, 2 * h, 2 * w, 4, dtype=q.dtype, device=q.device)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + 4]
    return out


# ------------------------------------------------------------------------------------------------ softmax_loss, flat and quad
@pytest.mark.parametrize("name", FORM_NAMES)
@pytest.mark.parametrize("C", [3, 2, 4])
def test_softmax_class_loss_flat_against_the_restatement(name, C):
    from ultrasound_modeling_amd import ops
    B, H, W, inv = 2, 9, 11, 0.25
    w, gamma, factor = R.form(name, C)
    logits, y = R.flat_inputs(C, B, H, W)
    r = R.from_logits(logits, y, w, gamma, factor, inv)
    lg = torch.zeros(B, H, W, 4)
    lg[..., :C] = logits.float()
    probs = torch.empty(B, H, W, C, device=DEV)
    loss = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl = ops.new_act(B, H, W, 8, DEV)
    ops.softmax_loss(lg.to(DEV), y.float().to(DEV), probs, loss, dl, HW=H * W, C_classes=C, inv_global_batch=inv, class_loss=_cl(w, gamma, factor))
    torch.cuda.synchronize()
    print(f"\n  {name} C={C}: probs rel {rel(probs, r['probs']):.2e}, loss {loss[0].item():.6f} vs {r['loss'].item():.6f}", end="")
    assert rel(probs, r["probs"]) < 1e-5
    assert abs(loss[0].item() - r["loss"].item()) <= 1e-5 * abs(r["loss"].item())
    assert loss[1].item() == 0                                # the ticket counter is back at zero
    assert dl[..., C:].abs().max().item() == 0
    _check_dlogits(f"flat {name} C={C}", dl[..., :C], r, w, factor, inv, forced=(0, 0, 0))
    # probabilities only (no labels): the same bits, nothing else written
    p2 = torch.empty_like(probs)
    ops.softmax_loss(lg.to(DEV), None, p2, None, None, HW=H * W, C_classes=C, class_loss=_cl(w, gamma, factor))
    assert torch.equal(p2, probs)


@pytest.mark.parametrize("name", FORM_NAMES)
@pytest.mark.parametrize("C", [3, 4])
def test_softmax_class_loss_quad_layout_against_the_restatement(name, C):
    from ultrasound_modeling_amd import ops
    B, H, W, inv = 2, 10, 12, 1.0 / 7.0
    w, gamma, factor = R.form(name, C)
    logits, y = R.flat_inputs(C, B, H, W)
    r = R.from_logits(logits, y, w, gamma, factor, inv)
    lq = _to_quad(logits.float()).to(DEV)
    probs = torch.empty(B, H, W, C, device=DEV)
    loss = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl = ops.new_act(B, H // 2, W // 2, 16, DEV)
    ops.softmax_loss(lq, y.float().to(DEV), probs, loss, dl, HW=H * W, C_classes=C, inv_global_batch=inv, quad_w=W, class_loss=_cl(w, gamma, factor))
    torch.cuda.synchronize()
    assert rel(probs, r["probs"]) < 1e-5
    assert abs(loss[0].item() - r["loss"].item()) <= 1e-5 * abs(r["loss"].item())
    d4 = _from_quad(dl)
    if C < 4:
        assert d4[..., C:].abs().max().item() == 0            # the pad classes of every parity slot
    _check_dlogits(f"quad {name} C={C}", d4[..., :C], r, w, factor, inv, forced=(0, 0, 0))


# ------------------------------------------------------------------------------------------------ the fused head
HEAD_CASES = [(2, 32, 32, 3, 3, 72), (1, 20, 36, 3, 3, 16), (3, 16, 5, 3, 3, 72), (2, 48, 16, 2, 4, 40), (1, 64, 64, 4, 3, 16)]


def _head(gen, B, h, w, C, k, cin):
    from test_gpu_ops import finalize, rnd, to_dev_padded
    from ultrasound_modeling_amd.layers import Conv2DTranspose, QuadHead
    head = Conv2DTranspose(cin, C, k)
    q = QuadHead(head)
    finalize(head)
    head.kernel.data.copy_(rnd(gen, k, k, C, cin, scale=1.0 / math.sqrt(k * k * cin)))
    head.bias.data.copy_(rnd(gen, C, scale=0.5))
    q.on_finalize(DEV)
    xd = to_dev_padded(rnd(gen, B, h, w, cin))
    y = torch.softmax(torch.randn(B, 2 * h, 2 * w, C, generator=gen), -1).to(DEV)
    return q, xd, y


@pytest.mark.parametrize("name", FORM_NAMES)
@pytest.mark.parametrize("B,h,w,C,k,cin", HEAD_CASES)
def test_fused_head_class_loss_equals_its_three_launches_and_the_restatement(name, B, h, w, C, k, cin):
    from ultrasound_modeling_amd import ops
    gen = torch.Generator().manual_seed(4321)
    wts, gamma, factor = R.form(name, C)
    cl = _cl(wts, gamma, factor)
    q, xd, y = _head(gen, B, h, w, C, k, cin)
    inv = 1.0 / 7.0
    # unfused: bias expand + conv (fp32 quad logits) + softmax_loss with the same class loss
    logits = q.forward(xd)
    probs_u = torch.empty(B, 2 * h, 2 * w, C, device=DEV)
    loss_u = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl_u = ops.new_act(B, h, w, 16, DEV)
    ops.softmax_loss(logits, y, probs_u, loss_u, dl_u, HW=4 * h * w, C_classes=C, inv_global_batch=inv, quad_w=2 * w, class_loss=cl)
    probs_f = torch.empty_like(probs_u)
    loss_f = torch.zeros(ops.ACC_FLOATS, device=DEV)
    dl_f = ops.new_act(B, h, w, 16, DEV)
    took = q.forward_loss(xd, y, probs_f, loss_f, dl_f, label_smoothing=0.1, clip_eps=1e-7, inv_global_batch=inv, class_loss=cl)
    if xd.shape[-1] not in (16, 72):
        assert not took           # no instantiation for this input width: nothing launched, the caller runs the three launches
        return
    assert took
    probs_n = torch.empty_like(probs_u)
    assert q.forward_loss(xd, None, probs_n, None, None, class_loss=cl)            # probabilities only
    torch.cuda.synchronize()
    assert rel(probs_f, probs_u) < 1e-5 and torch.equal(probs_n, probs_f)
    assert abs(loss_f[0].item() - loss_u[0].item()) <= 1e-5 * abs(loss_u[0].item())
    assert rel(dl_f, dl_u) < REL_BF16
    d4 = _from_quad(dl_f)
    if C < 4:
        assert d4[..., C:].abs().max().item() == 0
    # against the restatement, from the fp32 logits of the unfused conv (the fused MFMA sum differs from them by fp32 summation order)
    r = R.from_logits(_from_quad(logits)[..., :C].double().cpu(), y.double().cpu(), wts, gamma, factor, inv)
    assert rel(probs_f, r["probs"]) < 1e-5
    assert abs(loss_f[0].item() - r["loss"].item()) <= 1e-5 * abs(r["loss"].item())
    _check_dlogits(f"fused head {name} {B}x{h}x{w} C={C} cin={cin}", d4[..., :C], r, wts, factor, inv)


# ------------------------------------------------------------------------------------------------ loss_from_probs
@pytest.mark.parametrize("name", FORM_NAMES)
def test_class_loss_from_probabilities_scalar_and_map(name):
    from ultrasound_modeling_amd import ops
    w, gamma, factor = R.FORMS[name]
    g = torch.Generator().manual_seed(11)
    B, H, W = 3, 9, 11
    probs = torch.softmax(3 * torch.randn(B, H, W, 3, generator=g, dtype=torch.float64), -1)
    probs[0, 0, 0] = torch.tensor([1.0, 0.0, 0.0])                                          # both clip constants
    probs = (probs * (0.5 + torch.rand(B, H, W, 1, generator=g, dtype=torch.float64))).clamp(max=1.0).float().double()   # not normalised, and not divided
    y = torch.softmax(2 * torch.randn(B, H, W, 3, generator=g, dtype=torch.float64), -1).float().double()
    y0 = y.float().to(DEV)
    yd = y0.clone()
    cl = _cl(w, gamma, factor)
    loss = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.loss_from_probs(probs.float().to(DEV), yd, loss, HW=H * W, C_classes=3, inv_global_batch=0.25, class_loss=cl)
    lmap = torch.empty(H * W, device=DEV)
    ops.loss_from_probs(probs.float().to(DEV), yd, lmap, HW=H * W, C_classes=3, inv_global_batch=0.25, class_loss=cl, as_map=True)
    torch.cuda.synchronize()
    want_s = R.scalar(y, probs, w, gamma, factor, 4).item()
    want_m = R.loss_map(y, probs, w, gamma, factor)
    print(f"\n  {name}: scalar {loss[0].item():.6f} vs {want_s:.6f}, map rel {rel(lmap.reshape(H, W), want_m):.2e}", end="")
    assert math.isfinite(loss[0].item()) and abs(loss[0].item() - want_s) <= 1e-5 * abs(want_s)
    assert rel(lmap.reshape(H, W), want_m) < 1e-5
    assert torch.equal(yd, y0)                                                              # the labels are left as they were


# ------------------------------------------------------------------------------------------------ against loss_kind 0
def test_uniform_class_loss_coincides_with_the_cce_launch():
    """w = 1/3, factor 3, gamma 0 against CategoricalCrossentropy (loss_kind 0) on the same logits: softmax rows sum to one, so away from the
    clip the two losses are the same function."""
    from ultrasound_modeling_amd import ops
    B, H, W = 2, 9, 11
    g = torch.Generator().manual_seed(12)
    lg = torch.zeros(B, H, W, 4)
    lg[..., :3] = 3 * torch.randn(B, H, W, 3, generator=g)
    y = torch.softmax(2 * torch.randn(B, H, W, 3, generator=g), -1).to(DEV)
    out = []
    for cl in (None, _cl([1.0 / 3] * 3, 0.0, 3.0)):
        probs = torch.empty(B, H, W, 3, device=DEV)
        loss = torch.zeros(ops.ACC_FLOATS, device=DEV)
        dl = ops.new_act(B, H, W, 8, DEV)
        ops.softmax_loss(lg.to(DEV), y, probs, loss, dl, HW=H * W, C_classes=3, inv_global_batch=0.25, class_loss=cl)
        out.append((probs, loss[0].item(), dl))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0])
    assert abs(out[1][1] - out[0][1]) <= 1e-5 * abs(out[0][1])
    assert rel(out[1][2], out[0][2]) < REL_BF16


# ------------------------------------------------------------------------------------------------ the model
def _arch_b(seed=3, **kw):
    """tests/test_gpu_step.py::_arch_b with the loss keywords."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True).items()}
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1, learning_rate=1e-3, **kw)
    net.load_params(P)
    return net


def _batches(n, B, H, W):
    return [tuple(t for t in O.synthetic_batch(B, H, W, 1, seed=40 + i)) for i in range(n)]


def _model_form(net):
    cl = net._seg_loss.class_loss
    return list(cl.w)[:net.num_classes], cl.gamma, cl.factor


def test_the_default_loss_did_not_move():
    a, b = _arch_b(), _arch_b(loss="cce")
    assert a._seg_loss.class_loss is None and b._seg_loss.class_loss is None and a.loss_name == b.loss_name == "cce"
    assert a.alpha == 2 and a.class_factor == [0.06329, 0.027567, 0.90914]
    for x, y in _batches(2, 2, 64, 64):
        la, pa = a.train_step(x, y.float())
        lb, pb = b.train_step(x, y.float())
        torch.cuda.synchronize()
        assert la.item() == lb.item() and torch.equal(pa, pb)
    assert torch.equal(a.flat.flat, b.flat.flat)


@pytest.mark.parametrize("loss", ["my_loss_cat", "focal"])
def test_arch_b_steps_with_the_class_loss(loss):
    net = _arch_b(loss=loss)
    w, gamma, factor = _model_form(net)
    want_form = ([pytest.approx(v) for v in R.CLASS_FACTOR], 0.0, 3.0) if loss == "my_loss_cat" else ([1.0] * 3, 2.0, 1.0)
    assert (w, gamma, factor) == want_form
    x, y = _batches(1, 2, 64, 64)[0]
    l, probs = net.step(x, y.float())
    torch.cuda.synchronize()
    want = R.scalar(y, probs.double().cpu(), w, gamma, factor, net.batch_size).item()
    print(f"\n  {loss}: step loss {l.item():.6f}, restatement on its probabilities {want:.6f}", end="")
    assert abs(l.item() - want) <= 2e-5 * abs(want)
    # compute_loss follows loss=; my_loss_cat is the committed form whatever loss= says
    got = net.compute_loss(y.float(), probs)
    assert got.shape == () and abs(got.item() - want) <= 2e-5 * abs(want)
    cce = _arch_b().compute_loss(y.float(), probs).item()
    assert abs(got.item() - cce) > 1e-2 * abs(cce)
    y_dev = y.float().to(DEV)
    y_keep = y_dev.clone()
    m = net.my_loss_cat(y_dev, probs)
    assert tuple(m.shape) == (64, 64) and m.dtype == torch.float32
    assert rel(m, R.my_loss_cat(y, probs.double().cpu())) < 1e-5
    assert torch.equal(y_dev, y_keep)


@pytest.mark.parametrize("loss", ["my_loss_cat", "focal"])
def test_graph_replay_equals_eager_with_the_class_loss(loss):
    from test_gpu_step import _assert_same_state, _state
    eager, graph = _arch_b(loss=loss), _arch_b(loss=loss)
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


@pytest.mark.parametrize("loss", ["my_loss_cat", "focal"])
def test_the_class_loss_falls_on_one_fixed_batch(loss):
    net = _arch_b(loss=loss)
    x, y = _batches(1, 2, 64, 64)[0]
    losses = []
    for _ in range(20):
        l, _p = net.train_step(x, y.float())
        losses.append(l.item())
    print(f"\n  {loss}: {losses[0]:.4f} -> {losses[-1]:.4f}", end="")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_weighted_focal_and_focal_gamma_reach_the_kernel():
    net = _arch_b(loss="focal", class_factor=[0.2, 0.3, 0.5], focal_gamma=1.5)
    assert _model_form(net) == ([pytest.approx(0.2), pytest.approx(0.3), pytest.approx(0.5)], 1.5, 3.0)
    x, y = _batches(1, 2, 64, 64)[0]
    l, probs = net.step(x, y.float())
    want = R.scalar(y, probs.double().cpu(), [0.2, 0.3, 0.5], 1.5, 3.0, 2).item()
    assert abs(l.item() - want) <= 2e-5 * abs(want)


def test_transunet_variant_takes_the_mean_over_the_pixels():
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer
    H, W, B = 64, 128, 2
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=21, perturb=True, use_vit=True, transunet=True).items()}
    net = VisionTransformer(img_size=(H, W), batch_size=B, in_channels=1, loss="my_loss_cat")
    net.load_params(P)
    x, y = O.synthetic_batch(B, H, W, 1, seed=5)
    l, probs = net.step(x, y.float())
    torch.cuda.synchronize()
    want = R.scalar(y, probs.double().cpu(), *R.FORMS["my_loss_cat"], B * H * W).item()          # TBI_TransUNet.py:546: mean over B*H*W pixels
    assert abs(l.item() - want) <= 2e-5 * abs(want)
    l2, _ = net.step(x, y.float(), train=True)
    assert l2.item() == l.item()


def test_constructor_refuses_bad_loss_arguments():
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    mk = functools.partial(VisionTransformer, 2, (64, 64), in_channels=1)
    for kw in (dict(loss="dice"), dict(loss="my_loss_cat", class_factor=[0.5, 0.5]), dict(loss="focal", class_factor=[1.0] * 4),
               dict(loss="focal", focal_gamma=0.5), dict(loss="focal", focal_gamma=9.0), dict(loss="cce", focal_gamma=2.0),
               dict(loss="my_loss_cat", class_factor=[0.1, -0.2, 0.3]), dict(loss="my_loss_cat", num_classes=2)):
        with pytest.raises(ValueError):
            mk(**kw)


# ------------------------------------------------------------------------------------------------ two ranks
def test_two_gloo_ranks_with_my_loss_cat_equal_the_simulation_bit_for_bit(tmp_path, monkeypatch):
    """tests/test_gpu_mainparallel.py's world of two (gloo, both ranks on device 0) with ``main(..., loss="my_loss_cat")`` against its
    two-instance eager simulation built with the same loss."""
    import test_gpu_mainparallel as MP
    import ultrasound_modeling_amd.VisionTransformer as V
    train, val = MP._arrays(MP.N_TRAIN, seed=1), MP._arrays(MP.N_TEST, seed=2)
    np.save(tmp_path / "train.npy", train)
    np.save(tmp_path / "val.npy", val)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "USSEG_DP_CHUNKS")}
    env.update(USSEG_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc_per_node", "2", "--master_addr", "127.0.0.1",
                        "--master_port", str(MP._free_port()), os.path.abspath(__file__), str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = [torch.load(tmp_path / f"rank{k}.pt", weights_only=False) for k in range(2)]
    assert d[0]["graph"] and d[1]["graph"] and d[0]["loss_name"] == "my_loss_cat"
    assert torch.equal(d[0]["state"]["flat"], d[1]["state"]["flat"]), "replicas diverged"
    monkeypatch.setattr(V, "VisionTransformer", functools.partial(V.VisionTransformer, loss="my_loss_cat"))     # the simulation's two instances
    want, history = MP._simulate(train, val)
    for k in range(2):
        assert MP._first_difference(d[k]["state"], want[k]) is None, (k, MP._first_difference(d[k]["state"], want[k]))
    MP._same_history(d[0]["history"], history)
    MP._same_history(d[1]["history"], history)
    monkeypatch.undo()
    cce, _ = MP._simulate(train, val)                                                    # and the loss did change the training
    assert not torch.equal(cce[0]["flat"], want[0]["flat"])


def _rank(tmp):
    import torch.distributed as dist
    import test_gpu_mainparallel as MP
    from ultrasound_modeling_amd.MainParallel import main
    net, proc = main(os.path.join(tmp, "train.npy"), os.path.join(tmp, "val.npy"), None, epochs=MP.EPOCHS, batch_size=MP.B, use_vit=False,
                     seed=MP.SEED, loss="my_loss_cat")
    rank = dist.get_rank()
    torch.save({"state": MP._state(net), "history": proc.history, "graph": net._graph is not None, "loss_name": net.loss_name},
               os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    _rank(sys.argv[1])
