"""The distance maps, the boundary term and the surface scores on the GPU (usseg.h: usseg_sdf_labels, usseg_surface_dist, UssegBoundaryLoss;
csrc/sdf.hip, csrc/overlap_loss.hip) against the fp64 restatement (tests/boundary_restatement.py).

Bounds.
  * ``sdf_labels``: every element bit for bit - the restatement's fp64 value (the square root of the exact integer; 1 minus it inside the mask)
    rounded once to fp32.
  * ``surface_dist``: the int64 counters equal; the fp64 sums within 1e-12 relative of ``math.fsum`` (order-of-summation slack of at most 20 480
    fp64 terms: 20 480 * 2^-53 = 2.3e-12 would be the worst chain, the tree is far shorter) and bitwise equal from run to run.
  * The loss pair.  With wb = 0 everything equals the plain pair bit for bit.  Otherwise L_B (acc[12]) is a sum of SIGNED terms u_c*p_c*phi_c, so
    its error is relative to the sum of their magnitudes: |L_B - ref| <= gamma_d * kb * sum |u_c*p_c*phi_c| with tests/test_gpu_overlap_loss.py's
    gamma_d = d*u/(1 - d*u), u = 2^-24, and d = ``R.sum_depth(M)`` (its grid rule: the same reduction carries this total) - 1 (no p*y product)
    + 2 (the products p*phi and u*(.)) + C (the class sum of a pixel) + 3 (the host's rounding of ov_scale/M, wb times it, times the total).
    acc[0]: that file's 1e-5 relative bar for the overlap (+ CCE) part, plus the L_B bound, plus one rounding of the final sum.
    dlogits: that file's rule, |dl - ref| <= 4 * 2^-8 * mag + tiny, with mag carrying |kb*u_c*phi_c| as one more term of G_c and tiny unchanged; no
    wider slack was needed for the extra summand.  Without a CCE term no element is excused; with one, that file's cap (1e-3 of the pixels at a
    clip edge) holds and the inputs have none.
  * ov_scale = 0.5: the boundary part of the gradient is acc[13]*u_c*phi_c(m) with u and phi independent of ov_scale, so it is checked on the
    coefficient acc[13] (and on L_B, acc[12]): within one fp32 ulp of half the ov_scale = 1 value.
"""
import csv
import functools
import math
import types

import numpy as np
import pytest
import torch

import boundary_restatement as BR
import overlap_restatement as R
from route_probe import assert_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
U_BF16 = 2.0 ** -8
NEXT_HALF = np.nextafter(np.float32(0.5), np.float32(1.0))


# ------------------------------------------------------------------------------------------------ sdf_labels
def _plane(kind, H, W, rng):
    """One planted plane of labels, fp32 [H,W]."""
    p = np.zeros((H, W), dtype=np.float32)
    if kind == "empty":
        pass
    elif kind == "full":
        p[:] = 1.0
    elif kind == "corners":
        p[0, 0] = p[0, W - 1] = p[H - 1, 0] = p[H - 1, W - 1] = 1.0
    elif kind == "checker":
        p[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = 1.0
    elif kind == "row":
        p[H // 2, :] = 1.0
    elif kind in ("sparse", "dense", "blobs"):        # soft labels on both sides of the threshold
        m = rng.random((H, W)) < {"sparse": 0.02, "dense": 0.9, "blobs": 0.3}[kind]
        p = np.where(m, 0.5 + 0.5 * rng.random((H, W)) + 1e-3, 0.5 * rng.random((H, W))).astype(np.float32)
    elif kind == "half":                              # exactly 0.5 is OUTSIDE the mask
        p = np.where(rng.random((H, W)) < 0.3, 0.75, 0.5).astype(np.float32)
    elif kind == "next":                              # the next float above 0.5 is inside
        p = np.where(rng.random((H, W)) < 0.3, NEXT_HALF, np.float32(0.5)).astype(np.float32)
    elif kind == "nan":                               # NaN is outside
        p = np.where(rng.random((H, W)) < 0.3, 1.0, np.nan).astype(np.float32)
    else:
        raise KeyError(kind)
    return p


KINDS = ("empty", "full", "corners", "checker", "row", "sparse", "dense", "half", "next", "nan", "blobs", "blobs")


@functools.lru_cache(maxsize=None)
def _sdf_case(B, H, W, C, first):
    """Labels [B,H,W,C] whose planes cycle through KINDS from ``first``, and the restatement's phi rounded to fp32 (computed once)."""
    rng = np.random.default_rng(100 * H + W + first)
    y = np.empty((B, H, W, C), dtype=np.float32)
    kinds = []
    for b in range(B):
        for c in range(C):
            kinds.append(KINDS[(first + b * C + c) % len(KINDS)])
            y[b, :, :, c] = _plane(kinds[-1], H, W, rng)
    want = BR.phi(y).astype(np.float32)
    return y, want, kinds


def _run_sdf(y, want, kinds):
    from ultrasound_modeling_amd import ops
    yd = torch.from_numpy(y).to(DEV)
    B, H, W, C = y.shape
    phi = torch.full_like(yd, float("nan"))
    ws = torch.zeros(ops.sdf_ws_bytes(B, H, W, C), dtype=torch.uint8, device=DEV)
    ops.sdf_labels(yd, phi, ws)
    torch.cuda.synchronize()
    got = phi.cpu().numpy()
    for i, k in enumerate(kinds):
        b, c = divmod(i, C)
        bad = got[b, :, :, c].view(np.uint32) != want[b, :, :, c].view(np.uint32)
        assert not bad.any(), (k, (b, c), int(bad.sum()), np.argwhere(bad)[:3].tolist(), got[b, :, :, c][bad][:3], want[b, :, :, c][bad][:3])
    ops.sdf_labels(yd, phi, ws)                       # a second call into the same buffers: the same bits
    torch.cuda.synchronize()
    assert np.array_equal(phi.cpu().numpy().view(np.uint32), got.view(np.uint32))
    return got


# (the planes of the listed shapes cycle through the kinds from different starts, so that together they hold every kind at several sizes)
@pytest.mark.parametrize("B,H,W,C,first", [(2, 5, 7, 3, 0), (1, 1, 9, 2, 2), (1, 1, 9, 2, 5), (1, 9, 1, 2, 3), (1, 9, 1, 2, 8), (1, 33, 19, 3, 6),
                                           (3, 64, 48, 3, 0), (2, 256, 80, 3, 3)])
def test_sdf_labels_equals_the_restatement_bit_for_bit(B, H, W, C, first):
    _run_sdf(*_sdf_case(B, H, W, C, first))


def test_sdf_labels_every_planted_plane_in_one_batch():
    y, want, kinds = _sdf_case(4, 33, 19, 3, 0)
    assert set(kinds) == set(KINDS)
    got = _run_sdf(y, want, kinds)
    for i, k in enumerate(kinds):
        b, c = divmod(i, 3)
        if k in ("empty", "full"):
            assert not got[b, :, :, c].any()          # no boundary: phi = 0 everywhere
    # the definition's landmarks on the corner plane: the corner itself 0, its neighbour 1
    i = kinds.index("corners")
    b, c = divmod(i, 3)
    assert got[b, 0, 0, c] == 0.0 and got[b, 0, 1, c] == 1.0 and got[b, 1, 1, c] == np.float32(math.sqrt(2.0))


def test_sdf_labels_threshold_argument_and_four_classes():
    from ultrasound_modeling_amd import ops
    rng = np.random.default_rng(12)
    y = rng.random((2, 17, 70, 4)).astype(np.float32)          # W = 70: a second, partial 64-pixel word in every row
    want = BR.phi(y, 0.8).astype(np.float32)
    got = ops.sdf_labels(torch.from_numpy(y).to(DEV), threshold=0.8).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ surface_dist
def _mask_pair(case, H, W, rng):
    a, b = np.zeros((H, W), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    if case == "identical":
        a[:] = rng.random((H, W)) < 0.4
        a[H // 2, W // 2] = 1
        b[:] = a
    elif case == "disjoint":
        a[:, : max(W // 3, 1)] = 1
        b[:, W - max(W // 3, 1):] = 7                 # any nonzero byte is inside
        if W < 3:
            a[:], b[:] = 0, 0
            a[: max(H // 3, 1), :] = 1
            b[H - max(H // 3, 1):, :] = 1
    elif case == "one_empty":
        a[:] = rng.random((H, W)) < 0.5
        a[0, 0] = 1
    elif case == "both_empty":
        pass
    elif case == "full":
        a[:] = 1
        b[:] = rng.random((H, W)) < 0.3
        b[H - 1, W - 1] = 1
    elif case == "corners":
        a[0, 0] = 1
        b[H - 1, W - 1] = 1
    elif case == "random":
        a[:] = rng.random((H, W)) < 0.55
        b[:] = rng.random((H, W)) < 0.45
    elif case == "blobs":
        yy, xx = np.mgrid[0:H, 0:W]
        a[:] = ((yy - H * 0.4) ** 2 + (xx - W * 0.5) ** 2 <= (0.3 * min(H, W)) ** 2) | (rng.random((H, W)) < 0.01)
        b[:] = ((yy - H * 0.5) ** 2 / 4 + (xx - W * 0.4) ** 2 <= (0.25 * min(H, W)) ** 2) | (rng.random((H, W)) < 0.01)
    else:
        raise KeyError(case)
    return a, b


@functools.lru_cache(maxsize=None)
def _surface_case(cases, H, W):
    rng = np.random.default_rng(7 * H + W)
    pairs = [_mask_pair(c, H, W, rng) for c in cases]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ref = [BR.surface_counters(p[0], p[1]) for p in pairs]
    return a, b, ref


@pytest.mark.parametrize("cases,H,W", [(("identical", "disjoint", "one_empty"), 5, 7), (("corners", "random"), 1, 9), (("both_empty", "full"), 33, 19),
                                       (("random", "corners"), 64, 48), (("blobs",), 256, 80),
                                       (("identical", "disjoint", "one_empty", "both_empty", "full", "corners"), 33, 19), (("disjoint", "full", "corners"), 9, 1)])
def test_surface_dist_counters_equal_and_sums_reproducible(cases, H, W):
    from ultrasound_modeling_amd import ops
    a, b, ref = _surface_case(cases, H, W)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    c1, s1 = ops.surface_dist(ad, bd)
    c2, s2 = ops.surface_dist(ad, bd)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))          # bitwise from run to run
    for i, (cnt, dab, dba) in enumerate(ref):
        assert c1[i].tolist() == cnt, (cases[i], c1[i].tolist(), cnt)
        for got, d in ((s1[i, 0].item(), dab), (s1[i, 1].item(), dba)):
            want = math.fsum(d)
            print(f"\n  {cases[i]} {H}x{W}: sum {got!r} vs fsum {want!r} over {len(d)} distances", end="")
            assert abs(got - want) <= 1e-12 * abs(want)
    if "corners" in cases:
        i = cases.index("corners")
        assert c1[i].tolist() == [1, 1, (H - 1) ** 2 + (W - 1) ** 2, (H - 1) ** 2 + (W - 1) ** 2]


def test_metrics_surface_distances_gives_hd_and_assd():
    from ultrasound_modeling_amd.metrics import surface_distances
    cases = ("identical", "disjoint", "one_empty", "both_empty", "full", "corners")
    a, b, _ = _surface_case(cases, 33, 19)
    s = surface_distances(a, b.astype(bool))                                       # NumPy in, any dtype: != 0 is inside
    for i, c in enumerate(cases):
        hd, assd = BR.surface_scores(a[i], b[i])
        if math.isnan(hd):
            assert math.isnan(s["hd"][i]) and math.isnan(s["assd"][i]), c
        else:
            assert s["hd"][i] == hd and abs(s["assd"][i] - assd) <= 1e-12 * assd, (c, s["hd"][i], hd, s["assd"][i], assd)
    assert s["hd"][0] == 0.0 and s["hd"][5] == math.sqrt(32 ** 2 + 18 ** 2)
    assert set(s) == {"hd", "assd", "n_a", "n_b", "max_ab", "max_ba", "sum_ab", "sum_ba"}          # the raw counters too


# ------------------------------------------------------------------------------------------------ the loss pair
def _ol(cfg):
    from ultrasound_modeling_amd import ops
    return ops.overlap_loss(cfg["w"], cfg["alpha"], cfg["beta"], cfg["smooth"], cfg["power"], cfg["ov_weight"], cfg["ce_weight"])


def _from_quad(q):
    B, h, w, _ = q.shape
    out = torch.zeros(B, 2 * h, 2 * w, 4, dtype=q.dtype, device=q.device)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2, :] = q[..., 4 * (a * 2 + b):4 * (a * 2 + b) + 4]
    return out


@functools.lru_cache(maxsize=None)
def _loss_inputs(B, H, W, C=3):
    logits, _ = R.inputs(C, B, H, W)
    y = BR.labels(C, B, H, W)
    p32 = torch.softmax(logits.float(), -1).contiguous()
    return p32, y


def _run_pair(B, H, W, loss, wb, quad, ov_scale=0.5, inv=0.25, C=3, u=(0.0, 1.0, 1.0)):
    """-> cfg, p32, y, phi (device result, cpu), acc and dlogits of the boundary pair, and of the plain pair."""
    from ultrasound_modeling_amd import ops
    p32, y = _loss_inputs(B, H, W, C)
    cfg = R.config(loss, C, w=[(0.2 + 0.3 * c) / C for c in range(C)])
    pd, yd = p32.to(DEV), y.float().to(DEV)
    phi = ops.sdf_labels(yd)
    kw = dict(overlap=_ol(cfg), HW=H * W, C_classes=C, inv_global_batch=inv)
    shape = (B, H // 2, W // 2, 16) if quad else (B, H, W, 8)
    out = []
    for boundary in (True, False):
        acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
        dl = torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)     # every element must be written
        if boundary:
            wbd = torch.tensor([wb], dtype=torch.float32, device=DEV)
            bl = ops.boundary_loss(u)
            ops.overlap_boundary_loss_sums(pd, yd, phi, acc, boundary=bl, wb=wbd, ov_scale=ov_scale, **kw)
            ops.overlap_boundary_loss_bwd(pd, yd, phi, acc, dl, boundary=bl, quad_w=W if quad else 0, **kw)
        else:
            ops.overlap_loss_sums(pd, yd, acc, ov_scale=ov_scale, **kw)
            ops.overlap_loss_bwd(pd, yd, acc, dl, quad_w=W if quad else 0, **kw)
        torch.cuda.synchronize()
        out += [acc.cpu(), dl.cpu()]
    return (cfg, p32, y, phi.cpu()) + tuple(out)


PAIR_SHAPES = [(2, 16, 16), (4, 64, 48)]


@pytest.mark.parametrize("quad", [False, True], ids=["flat", "quad"])
@pytest.mark.parametrize("loss", ["dice", "dice_ce"])
@pytest.mark.parametrize("B,H,W", PAIR_SHAPES)
def test_zero_boundary_weight_equals_the_plain_pair_bit_for_bit(B, H, W, loss, quad):
    cfg, p32, y, phi, acc_b, dl_b, acc_p, dl_p = _run_pair(B, H, W, loss, 0.0, quad)
    assert acc_b[0].view(torch.int32).item() == acc_p[0].view(torch.int32).item()
    assert torch.equal(dl_b.view(torch.int16), dl_p.view(torch.int16))
    assert torch.equal(acc_b[2:12], acc_p[2:12]) and torch.equal(acc_b[16:32], acc_p[16:32])
    assert acc_b[12].item() == 0.0 and acc_b[13].item() == 0.0 and acc_b[1].item() == 0.0


def _lb_bound(M, C):
    d = R.sum_depth(M)[0] - 1 + 2 + C + 3
    u = 2.0 ** -24
    return d * u / (1.0 - d * u)


@pytest.mark.parametrize("quad", [False, True], ids=["flat", "quad"])
@pytest.mark.parametrize("wb", [0.01, 1.0])
@pytest.mark.parametrize("loss", ["dice", "dice_ce"])
@pytest.mark.parametrize("B,H,W", PAIR_SHAPES)
def test_the_boundary_pair_against_the_restatement(B, H, W, loss, wb, quad):
    inv, ov_scale, C = 0.25, 0.5, 3
    u = (0.0, 1.0, 1.0)
    cfg, p32, y, phi, acc, dl, acc_p, _ = _run_pair(B, H, W, loss, wb, quad, ov_scale, inv)
    assert np.array_equal(phi.numpy().view(np.uint32), BR.phi(y.float().numpy()).astype(np.float32).view(np.uint32))
    wb32 = float(np.float32(wb))                                                   # the device float the kernel reads
    want = BR.restate_at(p32, y, phi.double(), cfg, u, wb32, inv, ov_scale)
    M = B * H * W
    lb_tol = _lb_bound(M, C) * want["lb_abs"]
    print(f"\n  {loss} wb={wb} {B}x{H}x{W}: L_B {acc[12].item():.9g} vs {want['lb']:.9g} (|err| {abs(acc[12].item() - want['lb']):.2e}, bound {lb_tol:.2e}); "
          f"loss {acc[0].item():.8f} vs {want['loss']:.8f}", end="")
    assert abs(acc[12].item() - want["lb"]) <= lb_tol
    assert abs(acc[13].item() - want["kb"]) <= 3 * 2.0 ** -24 * want["kb"]
    plain = want["loss"] - want["lb"]
    assert abs(acc[0].item() - want["loss"]) <= 1e-5 * abs(plain) + lb_tol + 2.0 ** -23 * abs(want["loss"])
    assert acc[0].item() != acc_p[0].item() and acc[1].item() == 0.0
    assert torch.equal(acc[2:12], acc_p[2:12]) and torch.equal(acc[16:32], acc_p[16:32])      # every other slot as the plain pass leaves it
    if quad:
        d4 = _from_quad(dl.float())
        assert not torch.isnan(d4).any()
    else:
        d4 = dl.float()
        assert d4[..., 4:].abs().max().item() == 0
    assert d4[..., C:].abs().max().item() == 0                                     # pad channels exactly zero (the buffer started as NaN)
    tiny = 2.0 ** -20 * cfg["ov_weight"] * ov_scale * max(cfg["w"]) * cfg["power"] / want["D"].min().item()
    if cfg["ce_weight"] != 0.0:
        tiny += 2.0 ** -20 * cfg["ce_weight"] * inv
    skip = want["edge"]
    assert int(skip.sum()) <= (1e-3 * skip.numel() if cfg["ce_weight"] != 0.0 else 0)
    keep = ~skip
    assert_elementwise(d4[..., :C].double()[keep], want["dlogits"][keep], want["mag"][keep], U_BF16, 4.0, tiny=tiny, what=f"{loss} wb={wb} quad={quad}")
    # the summand is really there: the gradient moved against the plain pair's where phi is large
    assert not torch.equal(dl, _run_pair(B, H, W, loss, 0.0, quad, ov_scale, inv)[5])


def test_half_the_overlap_factor_halves_the_boundary_part():
    B, H, W = 4, 64, 48
    full = _run_pair(B, H, W, "dice", 0.01, False, ov_scale=1.0)[4]
    half = _run_pair(B, H, W, "dice", 0.01, False, ov_scale=0.5)[4]
    for slot in (12, 13):
        f, h = np.float32(full[slot].item()), np.float32(half[slot].item())
        assert f != 0 and abs(np.float64(h) - 0.5 * np.float64(f)) <= np.spacing(np.abs(np.float32(0.5) * f)), (slot, f, h)


def test_the_boundary_weight_is_read_from_the_device_at_run_time():
    """The same launch arguments, another value in the device float: the loss follows."""
    from ultrasound_modeling_amd import ops
    B, H, W, C = 2, 16, 16, 3
    p32, y = _loss_inputs(B, H, W, C)
    cfg = R.config("dice", C)
    pd, yd = p32.to(DEV), y.float().to(DEV)
    phi = ops.sdf_labels(yd)
    wbd = torch.tensor([0.25], device=DEV)
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device=DEV)
    call = lambda: ops.overlap_boundary_loss_sums(pd, yd, phi, acc, overlap=_ol(cfg), boundary=ops.boundary_loss([0.0, 1.0, 1.0]), wb=wbd, HW=H * W, C_classes=C)
    call()
    a = acc[:16].cpu().clone()
    wbd.fill_(0.5)
    call()
    b = acc[:16].cpu()
    assert b[12].item() == 2.0 * a[12].item() and b[13].item() == 2.0 * a[13].item() and a[12].item() != 0.0


# ------------------------------------------------------------------------------------------------ the model
def _arch_b(**kw):
    import test_gpu_overlap_loss as T
    return T._arch_b(**kw)


def _transunet(**kw):
    import test_gpu_overlap_loss as T
    return T._transunet(**kw)


def _batches(n, B=2, H=64, W=64):
    import test_gpu_overlap_loss as T
    return T._batches(n, B, H, W)


@pytest.mark.parametrize("make", [_arch_b, _transunet], ids=["archB", "transunet"])
def test_two_eager_steps_equal_two_graph_replays(make):
    from test_gpu_step import _assert_same_state, _state
    eager, graph = make(loss="dice", overlap={}, boundary={}), make(loss="dice", overlap={}, boundary={})
    bs = _batches(2)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    _assert_same_state(_state(eager), _state(graph), "capture must not change the training state")
    for i, (x, y) in enumerate(bs):
        l0, p0 = eager.train_step(x, y.float())
        l1, p1 = graph.train_step(x, y.float())
        torch.cuda.synchronize()
        assert math.isfinite(l0.item()) and l0.item() == l1.item(), (i, l0.item(), l1.item())
        assert torch.equal(p0, p1), i
        _assert_same_state(_state(eager), _state(graph), f"step {i}")
    assert graph._graph is not None and eager.boundary_weight == pytest.approx(0.01) and eager._loss[12].item() != 0.0


@pytest.mark.parametrize("make", [_arch_b, _transunet], ids=["archB", "transunet"])
def test_a_zero_weight_ends_on_the_parameters_of_no_boundary_at_all(make):
    a, b = make(loss="dice", overlap={}), make(loss="dice", overlap={}, boundary={"weight": 0})
    c = make(loss="dice", overlap={}, boundary={})
    for x, y in _batches(2):
        la, _ = a.train_step(x, y.float())
        lb, _ = b.train_step(x, y.float())
        c.train_step(x, y.float())
        assert la.item() == lb.item()
    torch.cuda.synchronize()
    assert torch.equal(a.flat.flat, b.flat.flat) and torch.equal(a.optimizer.m, b.optimizer.m)
    assert not torch.equal(a.flat.flat, c.flat.flat)                               # and the default weight does train differently
    assert a.boundary_weight is None and a.boundary_loss is None and b.boundary_weight == 0.0
    with pytest.raises(ValueError):
        a.set_boundary_weight(0.1)


@pytest.mark.parametrize("make", [_arch_b, _transunet], ids=["archB", "transunet"])
def test_set_boundary_weight_reaches_the_captured_graph_without_a_recapture(make):
    from test_gpu_step import _assert_same_state, _state
    graph, twin = make(loss="dice", overlap={}, boundary={}), make(loss="dice", overlap={}, boundary={"weight": 0.05})
    base = make(loss="dice", overlap={}, boundary={})
    (x, y), = _batches(1)
    graph.capture_graph(x, y.float())
    captured = graph._graph
    graph.set_boundary_weight(0.05)
    lg, _ = graph.train_step(x, y.float())
    lt, _ = twin.train_step(x, y.float())
    l0, _ = base.train_step(x, y.float())
    torch.cuda.synchronize()
    assert graph._graph is captured                                                # no recapture
    assert lg.item() == lt.item() and lg.item() != l0.item(), (lg.item(), lt.item(), l0.item())
    _assert_same_state(_state(graph), _state(twin), "replay with the new weight vs the eager twin")
    assert graph.boundary_weight == twin.boundary_weight == float(np.float32(0.05))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            graph.set_boundary_weight(bad)


def test_a_checkpoint_keeps_the_boundary_weight(tmp_path):
    a = _arch_b(loss="dice", overlap={}, boundary={"weight": 0.03})
    a.set_boundary_weight(0.07)
    a.save(str(tmp_path / "m.pt"))
    b = _arch_b(loss="dice", overlap={}, boundary={})
    assert b.boundary_weight == float(np.float32(0.01))
    b.load(str(tmp_path / "m.pt"))
    assert b.boundary_weight == float(np.float32(0.07))
    plain = _arch_b(loss="dice", overlap={})                                       # a model without the term loads the same file
    plain.load(str(tmp_path / "m.pt"))
    assert plain.boundary_weight is None and torch.equal(plain.flat.flat, a.flat.flat)


def test_compute_loss_follows_the_step():
    net = _arch_b(loss="dice", overlap={}, boundary={"weight": 0.5})
    (x, y), = _batches(1)
    l, probs = net.step(x, y.float())
    got = net.compute_loss(y.float(), probs)
    torch.cuda.synchronize()
    phi = BR.phi(y.float().numpy()).astype(np.float32)
    cfg = R.config("dice", 3)
    want = BR.loss(probs.double().cpu(), y, torch.from_numpy(phi).double(), cfg, BR.default_u(3), 0.5, 0.5, 1.0).item()
    assert abs(got.item() - want) <= 2e-5 * abs(want) and abs(l.item() - want) <= 2e-5 * abs(want), (l.item(), got.item(), want)


def test_mainnumpy_main_runs_with_the_boundary_term(tmp_path, monkeypatch, capsys):
    import re
    from test_gpu_metrics import _raw
    from ultrasound_modeling_amd import MainNumpy
    np.save(tmp_path / "train.npy", _raw(4, 64, 64, 10, seed=1))
    np.save(tmp_path / "val.npy", _raw(2, 64, 64, 10, seed=2))
    monkeypatch.setattr(MainNumpy, "input_size", (64, 64))
    net, proc = MainNumpy.main(str(tmp_path / "train.npy"), str(tmp_path / "val.npy"), None, epochs=1, batch_size=2, loss="dice", boundary={})
    out = capsys.readouterr().out
    m = re.search(r"Loss:([-+0-9.eE]+|nan|inf)", out)
    assert m and math.isfinite(float(m.group(1))), out
    assert net.boundary_weight == float(np.float32(0.01)) and proc.history[0]["phase"] == "train"


def test_the_ramp_adds_to_the_weight_after_each_epoch():
    from ultrasound_modeling_amd.MainNumpy import Process

    class Net:
        boundary_weight = 0.01

        def __init__(self):
            self.device = torch.device(DEV)
            self.sets = []

        def train_step(self, x, y):
            return torch.ones((), device=DEV), torch.full((1, 4, 4, 3), 1.0 / 3, device=DEV)

        def set_boundary_weight(self, w):
            self.sets.append(w)
            self.boundary_weight = w

    y = torch.zeros(1, 4, 4, 3, device=DEV)
    y[..., 0] = 1.0
    data = types.SimpleNamespace(next_train=lambda n: (torch.zeros(1, 4, 4, 1, device=DEV), y, True))
    net = Net()
    Process(batch_size=1, device=DEV).training(net, data, epochs=3, boundary_ramp=0.02)
    assert net.sets == pytest.approx([0.03, 0.05, 0.07])


# ------------------------------------------------------------------------------------------------ the evaluator
def _stub_result(N=4, H=33, W=19):
    from ultrasound_modeling_amd.TBIEvaluator import PolarResult
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    prob = np.stack([np.clip(1.2 - np.hypot(yy - H * (0.3 + 0.1 * i), xx - W * 0.5) / (0.2 * H), 0, 1) for i in range(N)]).astype(np.float32)
    label = np.stack([np.where(np.hypot(yy - H * 0.5, xx - W * (0.3 + 0.1 * i)) < 0.25 * W, 2.0, rng.choice([0.0, 1.0, 1.5], size=(H, W))) for i in range(N)])
    prob[N - 1] = 0.5                                                              # exactly the threshold: no predicted bleed in the last image
    z = np.zeros((N, H, W), np.float32)
    return PolarResult(z, prob, None, label, z, np.array([[f"img{i}"] for i in range(N)]))


def test_the_evaluators_surface_scores_equal_the_restatement():
    from ultrasound_modeling_amd import TBIEvaluator
    res = _stub_result()
    s = TBIEvaluator.surface_scores(res)
    for i in range(4):
        a, b = res.bleed_prob[i] > 0.5, res.label[i] > 1.5
        cnt, dab, dba = BR.surface_counters(a, b)
        hd, assd = BR.surface_scores(a, b)
        assert [s["n_a"][i], s["n_b"][i], s["max_ab"][i], s["max_ba"][i]] == cnt
        if math.isnan(hd):
            assert i == 3 and math.isnan(s["hd"][i]) and math.isnan(s["assd"][i])
        else:
            assert s["hd"][i] == hd and abs(s["assd"][i] - assd) <= 1e-12 * assd
    assert TBIEvaluator.surface_scores(res, threshold=0.9)["n_a"].tolist() != s["n_a"].tolist()


def test_the_surface_csv_has_one_row_per_image(tmp_path, monkeypatch, capsys):
    """``main --surface-csv``: the evaluator's run with its model, geometry and figures stubbed out (tests/test_gpu_cone.py runs those)."""
    from ultrasound_modeling_amd import TBIEvaluator as E
    res = _stub_result()
    np.save(tmp_path / "data.npy", np.zeros((4, 1, 1, 1, 12)))
    np.save(tmp_path / "paths.npy", res.names)
    monkeypatch.setattr(E.Cascade, "from_checkpoints", classmethod(lambda cls, *a, **k: types.SimpleNamespace(device=torch.device(DEV))))
    monkeypatch.setattr(E.ConeGeometry, "from_dir", classmethod(lambda cls, *a, **k: None))
    monkeypatch.setattr(E, "Polar_Model", lambda data, cascade, names=None, batch_size=16: res)
    monkeypatch.setattr(E, "Display", lambda *a, **k: [])
    path = tmp_path / "surface.csv"
    E.main([str(tmp_path / "data.npy"), str(tmp_path / "paths.npy"), str(tmp_path), str(tmp_path / "out"), "--bleed", "none.pt", "--surface-csv", str(path)])
    assert "wrote 4 surface-score rows" in capsys.readouterr().out
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["name", "hd", "assd", "n_pred", "n_label"] and len(rows) == 1 + 4
    s = E.surface_scores(res)
    for i, r in enumerate(rows[1:]):
        assert r[0] == str(res.names[i]) and int(r[3]) == s["n_a"][i] and int(r[4]) == s["n_b"][i]
        assert (math.isnan(float(r[1])) and math.isnan(s["hd"][i])) or float(r[1]) == s["hd"][i]
        assert (math.isnan(float(r[2])) and math.isnan(s["assd"][i])) or float(r[2]) == s["assd"][i]
