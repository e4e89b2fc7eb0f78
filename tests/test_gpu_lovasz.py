"""The device radix sort (usseg.h usseg_sort_pairs_u32) and the Lovasz-softmax loss built on it (UssegLovaszLoss, csrc/lovasz.hip) on the GPU:

  * the sort, exact against ``np.argsort(kind="stable")``: sizes around the wave (64) and the tile (T = USSEG_SORT_TILE), 1 / 3 / 4 segments,
    1 / 8 / 30 / 32 key bits, seven key patterns; three calls bit for bit; a workspace one byte short refused;
  * ``ops.lovasz_coeffs``: the foreground counts exact, ``g`` per element against the fp64 restatement (tests/lovasz_restatement.py);
  * ``ops.lovasz_loss_sums``: L_c, the scalar loss, the ticket, three calls bit for bit, M = 0;
  * ``ops.lovasz_loss_bwd``: ``dlogits`` per element, row and quad layouts, pad channels exactly zero; the CCE limit against the loss_kind 0 launch;
  * Arch B at 64x64 and the TransUNet variant with ``loss="lovasz"`` / ``"lovasz_ce"``: finite steps, the loss falls on a fixed batch, graph replay
    equals eager bit for bit, ``loss="cce"`` does not move, two gloo ranks equal the two-instance simulation bit for bit (an empty replica included).

Bounds.  Ranks and counts are exact integers (any correct sort gives the same permutation: the order is strict), so ``g`` carries only the
roundings of its closed form - at most six in fp32 (three conversions, a subtraction, a multiply, a divide): |g - ref| <= 8 * 2^-24 * ref.
L_c: every term e*g is non-negative, so the total is within gamma_d (``overlap_restatement.sum_bound``: the depth of the grid rule the sums pass
shares with the overlap losses) plus the per-term roundings (g's, e's, the product's: 10 * 2^-24) RELATIVE of the restatement.  Scalar loss: 1e-5
relative, the project's bar.  dlogits: |dl - ref| <= 4 * 2^-8 * mag + tiny (tests/test_gpu_overlap_loss.py's construction) with mag from the
restatement's term sizes S_c = |k_c|*g_c (+ the CCE term) carried through p_k*(G_k - sum_c G_c*p_c), and tiny = 2^-20 * max_c |k_c|*max_m g_c(m)
(+ 2^-20 * ce_weight*inv_global_batch): 2^-20 of the largest gradient term of the call.  With a CCE term a pixel within 2^-20 relative of a clip
constant may be left out (at most 1e-3 of the pixels); the gauss inputs have none (tests/test_cpu_lovasz.py).  Without one, none is left out.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lovasz_restatement as V
import overlap_restatement as R
from route_probe import assert_elementwise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
U_BF16 = 2.0 ** -8
T = 2048                                               # USSEG_SORT_TILE (tests/test_cpu_lovasz.py holds the header to it)
SHAPES = [(2, 256, 80), (1, 64, 47), (1, 9, 7), (1, 1, 1)]      # 20 tiles; 2 tiles, the last partly filled; one partial wave; one pixel
NAMES = ["lovasz", "lovasz_ce"]


def _ll(cfg):
    from ultrasound_modeling_amd import ops
    return ops.lovasz_loss(cfg["w"], cfg["lv_weight"], cfg["ce_weight"], cfg["threshold"], cfg["classes"])


def _cfg(loss, C, **kw):
    return V.config(loss, C, w=[0.2 + 0.3 * c for c in range(C)], lv_weight=0.7, **kw)


def _probs(logits):
    return torch.softmax(logits.float(), -1).contiguous()


# ------------------------------------------------------------------------------------------------ the sort
PATTERNS = ("uniform", "equal", "four", "ascending", "descending", "top digit", "bottom digit")


def _keys(pattern, S, n, rng):
    if pattern == "uniform":
        return rng.integers(0, 1 << 32, (S, n), dtype=np.uint64).astype(np.uint32)
    if pattern == "equal":
        return np.full((S, n), 0xDEADBEEF, dtype=np.uint32)
    if pattern == "four":
        return rng.choice(np.array([0x00000000, 0x00000001, 0x3F800000, 0xFFFFFFFF], dtype=np.uint32), (S, n))
    if pattern in ("ascending", "descending"):
        a = (np.arange(n, dtype=np.uint64) * ((1 << 32) // n)).astype(np.uint32)             # strictly increasing, every digit in use
        a = np.broadcast_to(a if pattern == "ascending" else a[::-1], (S, n))
        return np.ascontiguousarray(a)
    d = rng.integers(0, 256, (S, n), dtype=np.uint64).astype(np.uint32)
    return (d << np.uint32(24)) | np.uint32(0x00ABCDEF) if pattern == "top digit" else np.uint32(0x12345600) | d


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 40960])
def test_the_sort_is_numpys_stable_argsort(n):
    from ultrasound_modeling_amd import ops
    rng = np.random.default_rng(n)
    for S in (1, 3, 4):
        vals = rng.integers(0, 1 << 32, (S, n), dtype=np.uint64).astype(np.uint32)
        vd = torch.from_numpy(vals.view(np.int32)).to(DEV)
        ws = torch.empty(max(ops.sort_ws_bytes(S, n), 16), dtype=torch.uint8, device=DEV)
        for pattern in PATTERNS:
            keys = _keys(pattern, S, n, rng)
            kd = torch.from_numpy(keys.view(np.int32).copy()).to(DEV)
            for bits in (1, 8, 30, 32):
                ko, vo = ops.sort_pairs(kd, vd, bits, ws)
                runs = [(ko, vo)]
                if pattern == "uniform":                               # three calls, bit for bit
                    runs += [ops.sort_pairs(kd, vd, bits, ws) for _ in range(2)]
                    assert all(torch.equal(ko, a) and torch.equal(vo, b) for a, b in runs[1:]), (S, pattern, bits)
                low = keys & np.uint32((1 << bits) - 1) if bits < 32 else keys
                perm = np.argsort(low, axis=1, kind="stable")
                what = f"n={n} S={S} {pattern} key_bits={bits}"
                assert np.array_equal(ko.cpu().numpy().view(np.uint32), np.take_along_axis(keys, perm, 1)), what      # the full keys travel
                assert np.array_equal(vo.cpu().numpy().view(np.uint32), np.take_along_axis(vals, perm, 1)), what
                if pattern == "equal" or (pattern == "top digit" and bits <= 24):                                       # no key difference: input order
                    assert np.array_equal(vo.cpu().numpy().view(np.uint32), vals), what


def test_a_workspace_one_byte_short_is_refused_and_one_segment_may_be_flat():
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    n = 3 * T + 17
    k = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=DEV)
    v = torch.arange(n, dtype=torch.int32, device=DEV)
    need = ops.sort_ws_bytes(1, n)
    with pytest.raises(L.UssegError, match=f"the workspace holds {need - 1} bytes, {need} needed"):
        ops.sort_pairs(k, v, 32, torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    ko, vo = ops.sort_pairs(k, v, 32, torch.empty(need, dtype=torch.uint8, device=DEV))
    ku = k.cpu().numpy().view(np.uint32)
    perm = np.argsort(ku, kind="stable")
    assert np.array_equal(ko.cpu().numpy().view(np.uint32), ku[perm]) and np.array_equal(vo.cpu().numpy(), perm.astype(np.int32))


# ------------------------------------------------------------------------------------------------ the coefficients
def _coeffs(p32, y, cfg, H, W):
    from ultrasound_modeling_amd import ops
    C = p32.shape[-1]
    M = p32.numel() // C
    pd, yd = p32.to(DEV), y.float().to(DEV)
    g = torch.full_like(pd, float("nan"))                       # every element must be written
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(ops.lovasz_ws_bytes(M, C), 16), dtype=torch.uint8, device=DEV)
    ops.lovasz_coeffs(pd, yd, g, counts, ws, lovasz=_ll(cfg), HW=H * W, C_classes=C)
    return pd, yd, g, counts


def _check_g(what, g, counts, p32, y, cfg):
    C = p32.shape[-1]
    ref, cnt, _ = V.coeffs(p32.numpy(), y.numpy(), cfg["threshold"])
    assert counts.cpu().numpy()[:C].tolist() == cnt.tolist(), what
    got = g.double().cpu().numpy().reshape(-1, C)
    err = np.abs(got - ref)
    worst = (err / np.maximum(ref, 1e-300)).max()
    print(f"\n  {what}: counts {cnt.tolist()}, worst g error {worst / 2.0 ** -24:.2f} * 2^-24 of g", end="")
    assert (err <= 8 * 2.0 ** -24 * ref).all(), what


@pytest.mark.parametrize("C", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_coefficients_per_element_and_counts_exactly(B, H, W, C):
    for kind in V.KINDS:
        logits, y = V.inputs(kind, C, B, H, W)
        cfg = _cfg("lovasz", C)
        p32 = _probs(logits)
        _, _, g, counts = _coeffs(p32, y, cfg, H, W)
        _check_g(f"{kind} C={C} {B}x{H}x{W}", g, counts, p32, y, cfg)


def test_coefficients_at_the_training_steps_size_and_another_threshold():
    B, H, W, C = 16, 256, 80, 3
    logits, y = V.inputs("gauss", C, B, H, W)
    cfg = _cfg("lovasz", C, threshold=0.4)
    p32 = _probs(logits)
    _, _, g, counts = _coeffs(p32, y, cfg, H, W)
    _check_g(f"gauss C={C} {B}x{H}x{W} thr 0.4", g, counts, p32, y, cfg)


# ------------------------------------------------------------------------------------------------ the sums
def _sums(p32, y, cfg, H, W, inv, ov_scale, calls=1):
    from ultrasound_modeling_amd import ops
    C = p32.shape[-1]
    pd, yd, g, counts = _coeffs(p32, y, cfg, H, W)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    runs = []
    for _ in range(calls):
        ops.lovasz_loss_sums(pd, yd, g, counts, acc, lovasz=_ll(cfg), HW=H * W, C_classes=C, ov_scale=ov_scale, inv_global_batch=inv)
        torch.cuda.synchronize()
        runs.append(acc[:32].cpu().clone())
        assert acc[1].item() == 0                              # the ticket counter is back at zero: no per-call zeroing
    return pd, yd, g, acc, runs


SUM_CASES = [(loss, classes, kind, C) + shp for loss, classes, kind in (("lovasz", "present", "gauss"), ("lovasz_ce", "all", "gauss"), ("lovasz_ce", "present", "absent"),
                                                                        ("lovasz", "all", "quantised"))
             for C in (3, 2, 4) for shp in SHAPES] + [("lovasz_ce", "present", "gauss", 3, 2, 256, 272), ("lovasz_ce", "present", "gauss", 3, 1, 768, 720)]


@pytest.mark.parametrize("loss,classes,kind,C,B,H,W", SUM_CASES)
def test_sums_against_the_restatement_and_bit_for_bit_over_three_calls(loss, classes, kind, C, B, H, W):
    M = B * H * W
    logits, y = V.inputs(kind, C, B, H, W)
    cfg = _cfg(loss, C, classes=classes)
    inv, ov_scale = 1.0 / 7.0, 0.5
    p32 = _probs(logits)
    want = V.restate_at(p32, y, cfg, inv, ov_scale)
    _, _, _, acc, runs = _sums(p32, y, cfg, H, W, inv, ov_scale, calls=3)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    got = runs[0].double()
    bound = R.sum_bound(M) + 10 * 2.0 ** -24
    err = ((got[16:16 + C] - want["L"]).abs() / want["L"]).max().item()
    print(f"\n  {loss} {classes} {kind} C={C} {B}x{H}x{W}: L_c rel err {err:.2e} (bound {bound:.2e})", end="")
    assert err <= bound
    k = torch.from_numpy(want["k"])
    assert ((got[4:4 + C] - k).abs() <= 4 * 2.0 ** -24 * k).all()                # three roundings: two products and the division by |S|
    print(f"; loss {got[0].item():.7f} vs {want['loss']:.7f}", end="")
    assert abs(got[0].item() - want["loss"]) <= 1e-5 * abs(want["loss"])


def test_no_class_present_gives_a_zero_loss_and_zero_coefficients():
    C, B, H, W = 3, 1, 64, 47
    logits, y = V.inputs("gauss", C, B, H, W)
    _, _, _, acc, runs = _sums(_probs(logits), torch.zeros_like(y), _cfg("lovasz", C), H, W, 0.25, 1.0)
    assert runs[0][0].item() == 0.0 and not runs[0][4:8].any()


def test_sums_of_no_pixels_give_a_zero_loss():
    """M = 0 through the C ABI (an empty tensor has no data pointer to pass): counts 0, loss 0, the ticket at zero, no backward launch."""
    import ctypes as C
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    acc[0] = 7.0
    buf = torch.zeros(16, device=DEV)
    counts = torch.full((4,), 5, dtype=torch.int32, device=DEV)
    d = L.LossDesc(0, 16, 3, 3, 8, 0, 0.1, 1e-7, 0.25, 0)
    ll = _ll(_cfg("lovasz_ce", 3))
    s = torch.cuda.current_stream().cuda_stream
    L.check(L.load().usseg_lovasz_coeffs(C.byref(d), ll, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), counts.data_ptr(), buf.data_ptr(), 64, s), "coeffs")
    L.check(L.load().usseg_lovasz_loss_sums(C.byref(d), ll, 1.0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), counts.data_ptr(), acc.data_ptr(), acc.numel(), s),
            "sums")
    L.check(L.load().usseg_lovasz_loss_bwd(C.byref(d), ll, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), acc.data_ptr(), acc.numel(), buf.data_ptr(), s), "bwd")
    torch.cuda.synchronize()
    assert acc[0].item() == 0.0 and acc[1].item() == 0.0 and counts[:3].tolist() == [0, 0, 0] and counts[3].item() == 5


# ------------------------------------------------------------------------------------------------ dlogits
def _to_quad_shape(B, H, W):
    return (B, H // 2, W // 2, 16)


def _from_quad(q):
    B, h, w, _ = q.shape
    out = torch.zeros(B, 2 * h, 2 * w, 4, dtype=q.dtype, device=q.device)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + 4]
    return out


def _run_both(loss, kind, classes, C, B, H, W, quad, inv=0.25, ov_scale=0.5):
    from ultrasound_modeling_amd import ops
    logits, y = V.inputs(kind, C, B, H, W)
    cfg = _cfg(loss, C, classes=classes)
    p32 = _probs(logits)
    pd, yd, g, acc, _ = _sums(p32, y, cfg, H, W, inv, ov_scale)
    dl = torch.full(_to_quad_shape(B, H, W) if quad else (B, H, W, 8), float("nan"), dtype=torch.bfloat16, device=DEV)   # every element must be written
    ops.lovasz_loss_bwd(pd, yd, g, acc, dl, lovasz=_ll(cfg), HW=H * W, C_classes=C, inv_global_batch=inv, quad_w=W if quad else 0)
    torch.cuda.synchronize()
    return cfg, p32, y, dl


def _check_dlogits(what, d, p32, y, cfg, inv, ov_scale):
    """d [B,H,W,C] against the restatement taken at the same fp32 probabilities."""
    p = p32.double()
    want = V.restate_at(p32, y, cfg, inv, ov_scale)
    G, S = want["G"], want["S"]
    ref = p * (G - (G * p).sum(-1, keepdim=True))
    tiny = 2.0 ** -20 * float((np.abs(want["k"]) * want["g"].reshape(-1, p.shape[-1]).max(0)).max())
    skip = torch.zeros(p.shape[:-1], dtype=torch.bool)
    if cfg["ce_weight"] != 0.0:
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


# lovasz_ce on the gauss inputs (no pixel at a clip edge); the Lovasz term alone also on ties, saturated probabilities and an absent class
DL_CASES = [("lovasz", "gauss", "present"), ("lovasz_ce", "gauss", "present"), ("lovasz_ce", "gauss", "all"), ("lovasz", "quantised", "present"),
            ("lovasz", "saturated", "all"), ("lovasz", "absent", "present")]


@pytest.mark.parametrize("loss,kind,classes", DL_CASES)
@pytest.mark.parametrize("C", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_dlogits_row_layout_per_element(loss, kind, classes, C, B, H, W):
    cfg, p32, y, dl = _run_both(loss, kind, classes, C, B, H, W, quad=False)
    assert dl[..., C:].float().abs().max().item() == 0                # pad channels exactly zero (and written: the buffer started as NaN)
    _check_dlogits(f"row {loss} {kind} {classes} C={C} {B}x{H}x{W}", dl[..., :C].float(), p32, y, cfg, 0.25, 0.5)


@pytest.mark.parametrize("loss,kind,classes", DL_CASES[:4])
@pytest.mark.parametrize("C", [3, 2, 4])
@pytest.mark.parametrize("B,H,W", [(2, 256, 80), (1, 64, 46), (3, 10, 6)])      # (the quad layout needs even H and W: 64x46 stands in for 64x47)
def test_dlogits_quad_layout_per_element(loss, kind, classes, C, B, H, W):
    cfg, p32, y, dl = _run_both(loss, kind, classes, C, B, H, W, quad=True)
    d4 = _from_quad(dl.float())
    assert not torch.isnan(d4).any()                                  # all 16 channels of every quad pixel were written
    if C < 4:
        assert d4[..., C:].abs().max().item() == 0                    # the pad classes of every parity slot
    _check_dlogits(f"quad {loss} {kind} {classes} C={C} {B}x{H}x{W}", d4[..., :C], p32, y, cfg, 0.25, 0.5)


@pytest.mark.parametrize("quad", [False, True])
def test_the_cce_limit_equals_the_existing_cce_launch(quad):
    """lv_weight = 0, ce_weight = 1: the loss and dlogits of the existing loss_kind 0 launch on the same logits, dlogits with the per-element bound."""
    from ultrasound_modeling_amd import ops
    C, B, H, W, inv = 3, 2, 64, 46, 0.25
    logits, y = V.inputs("gauss", C, B, H, W)
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
    cfg = V.config("lovasz_ce", C, lv_weight=0.0, ce_weight=1.0)
    g = torch.empty_like(probs)
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.lovasz_ws_bytes(B * H * W, C), dtype=torch.uint8, device=DEV)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    kw = dict(lovasz=_ll(cfg), HW=H * W, C_classes=C)
    ops.lovasz_coeffs(probs, yd, g, counts, ws, **kw)
    ops.lovasz_loss_sums(probs, yd, g, counts, acc, ov_scale=1.0, inv_global_batch=inv, **kw)
    dl1 = torch.full_like(dl0, float("nan"))
    ops.lovasz_loss_bwd(probs, yd, g, acc, dl1, quad_w=W if quad else 0, inv_global_batch=inv, **kw)
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
def _builders():
    import test_gpu_overlap_loss as OL
    return {"archB": OL._arch_b, "transunet": OL._transunet}, OL._batches


def _model_cfg(net):
    ll = net.lovasz_loss
    return dict(w=list(ll.w)[:net.num_classes], lv_weight=ll.lv_weight, ce_weight=ll.ce_weight, threshold=ll.threshold,
                classes="all" if ll.all_classes else "present")


@pytest.mark.parametrize("loss", NAMES)
@pytest.mark.parametrize("make", ["archB", "transunet"])
def test_the_model_steps_with_the_lovasz_loss_and_the_loss_falls(make, loss):
    """Eight steps on one fixed batch, the count tests/test_gpu_overlap_loss.py uses."""
    builders, batches = _builders()
    net = builders[make](loss=loss)
    x, y = batches(1, 2, 64, 64)[0]
    l, probs = net.step(x, y.float())
    torch.cuda.synchronize()
    inv = 1.0 / (2 * 64 * 64) if net.transunet else 0.5
    want = V.loss(probs.double().cpu(), y.double(), _model_cfg(net), inv, 1.0).item()
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


@pytest.mark.parametrize("loss", NAMES)
@pytest.mark.parametrize("make", ["archB", "transunet"])
def test_graph_replay_equals_eager_with_the_lovasz_loss(make, loss):
    from test_gpu_step import _assert_same_state, _state
    builders, batches = _builders()
    eager, graph = builders[make](loss=loss), builders[make](loss=loss, lovasz={})
    bs = batches(3, 2, 64, 64)
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
    x, y = batches(1, 1, 64, 64)[0]                                  # a short batch after the capture runs eagerly, through the same calls
    l0, _ = eager.train_step(x, y.float())
    l1, _ = graph.train_step(x, y.float())
    assert l0.item() == l1.item()


def test_the_default_loss_does_not_move_across_the_new_code():
    """loss="cce" built before and after a Lovasz model has been built and stepped: the same bits, and not one Lovasz buffer."""
    builders, batches = _builders()
    a = builders["archB"](loss="cce")
    d = builders["archB"](loss="lovasz_ce")
    bs = batches(2, 2, 64, 64)
    d.train_step(bs[0][0], bs[0][1].float())
    b = builders["archB"]()
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.seg_loss import LovaszLoss
    assert a.lovasz_loss is None and b.lovasz_loss is None and not isinstance(b._seg_loss, LovaszLoss) and a._loss.numel() == b._loss.numel() == ops.ACC_FLOATS
    for x, y in bs:
        la, pa = a.train_step(x, y.float())
        lb, pb = b.train_step(x, y.float())
        torch.cuda.synchronize()
        assert la.item() == lb.item() and torch.equal(pa, pb)
    assert torch.equal(a.flat.flat, b.flat.flat)
    assert not torch.equal(a.flat.flat, d.flat.flat)


# ------------------------------------------------------------------------------------------------ two ranks
def test_two_gloo_ranks_with_lovasz_ce_equal_the_simulation_bit_for_bit(tmp_path):
    """tests/test_gpu_overlap_loss.py's two-rank test with ``main(..., loss="lovasz_ce")``: nine images in batches of four, so the last step
    leaves rank 1 without an image; ranks and simulation each in a fresh process."""
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
    assert d[0]["graph"] and d[1]["graph"] and d[0]["loss_name"] == "lovasz_ce"
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
                     seed=MP.SEED, loss="lovasz_ce")
    rank = dist.get_rank()
    torch.save({"state": MP._state(net), "history": proc.history, "graph": net._graph is not None, "loss_name": net.loss_name},
               os.path.join(tmp, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _simulate(tmp):
    """``test_gpu_mainparallel._simulate`` with both instances built with ``loss="lovasz_ce"``."""
    import test_gpu_mainparallel as MP
    import ultrasound_modeling_amd.VisionTransformer as VT
    orig, made = VT.VisionTransformer, []

    def make(*a, **kw):
        made.append(orig(*a, loss="lovasz_ce", **kw))
        return made[-1]
    VT.VisionTransformer = make
    want, history = MP._simulate(np.load(os.path.join(tmp, "train.npy")), np.load(os.path.join(tmp, "val.npy")))
    assert len(made) == 2 and all(n.loss_name == "lovasz_ce" and n.lovasz_loss is not None for n in made), "the simulation did not train with lovasz_ce"
    torch.save({"want": want, "history": history}, os.path.join(tmp, "sim.pt"))


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    if sys.argv[2:] == ["simulate"]:
        _simulate(sys.argv[1])
    else:
        _rank(sys.argv[1])
