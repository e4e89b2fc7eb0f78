"""The distance maps, the boundary term and the surface scores without a GPU: the fp64 restatement (tests/boundary_restatement.py) against
SciPy and against hand answers, the C ABI (exported symbols, header text, struct layout, every argument check of the four entry points before
any launch), the constructor's and the command line's refusals, and the drivers' signatures."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

import boundary_restatement as BR
import overlap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement against SciPy
@pytest.mark.parametrize("H,W", [(5, 7), (33, 19), (64, 48), (1, 9)])
@pytest.mark.parametrize("density", [0.02, 0.3, 0.9])
def test_phi_equals_scipys_form_of_kervadecs_map_bit_for_bit(H, W, density):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1000 * H + W + int(100 * density))
    m = rng.random((H, W)) < density
    if not m.any():
        m[H // 2, W // 2] = True
    if m.all():
        m[0, 0] = False
    neg = ~m
    want = nd.distance_transform_edt(neg) * neg - (nd.distance_transform_edt(m) - 1) * m
    got = BR.phi_plane(m)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(BR.sq_transform(m), np.rint(nd.distance_transform_edt(neg) ** 2).astype(np.int64))


@pytest.mark.parametrize("H,W", [(5, 7), (33, 19), (1, 9), (9, 1)])
def test_surface_equals_the_mask_minus_its_binary_erosion(H, W):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(H * W)
    for density in (0.1, 0.6, 0.95, 1.0):
        m = rng.random((H, W)) < density
        want = m & ~nd.binary_erosion(m, structure=nd.generate_binary_structure(2, 1), border_value=0)
        assert np.array_equal(BR.surface(m), want)


def test_surface_distances_equal_scipys_transform_of_the_other_surface():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    a, b = rng.random((33, 19)) < 0.3, rng.random((33, 19)) < 0.2
    c, dab, dba = BR.surface_counters(a, b)
    sa, sb = BR.surface(a), BR.surface(b)
    assert np.array_equal(dab, nd.distance_transform_edt(~sb)[sa]) and np.array_equal(dba, nd.distance_transform_edt(~sa)[sb])
    hd, assd = BR.surface_scores(a, b)
    assert hd == max(dab.max(), dba.max()) and abs(assd - 0.5 * (dab.mean() + dba.mean())) <= 1e-14 * assd


# ------------------------------------------------------------------------------------------------ hand answers
def test_a_single_pixel():
    m = np.zeros((5, 7), dtype=bool)
    m[2, 3] = True
    d2 = BR.sq_transform(m)
    yy, xx = np.mgrid[0:5, 0:7]
    assert np.array_equal(d2, (yy - 2) ** 2 + (xx - 3) ** 2)
    p = BR.phi_plane(m)
    assert p[2, 3] == 0.0 and p[2, 4] == 1.0 and p[0, 0] == math.sqrt(13.0)      # the pixel itself is the first inside: 0; its neighbour 1
    assert np.array_equal(BR.surface(m), m)                                       # its own surface
    c, dab, dba = BR.surface_counters(m, m)
    assert c == [1, 1, 0, 0] and dab.tolist() == [0.0] and BR.surface_scores(m, m) == (0.0, 0.0)


@pytest.mark.parametrize("H,W", [(5, 7), (1, 9), (33, 19)])
def test_two_opposite_corners(H, W):
    a, b = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    a[0, 0] = True
    b[H - 1, W - 1] = True
    c, dab, dba = BR.surface_counters(a, b)
    want = (H - 1) ** 2 + (W - 1) ** 2
    assert c == [1, 1, want, want]
    hd, assd = BR.surface_scores(a, b)
    assert hd == math.sqrt(want) and assd == math.sqrt(want)


def test_identical_masks_have_distance_zero():
    rng = np.random.default_rng(4)
    m = rng.random((9, 11)) < 0.4
    c, dab, dba = BR.surface_counters(m, m)
    assert c[0] == c[1] > 0 and c[2] == c[3] == 0 and not dab.any()
    assert BR.surface_scores(m, m) == (0.0, 0.0)


def test_empty_and_full_planes():
    e, f = np.zeros((4, 6), dtype=bool), np.ones((4, 6), dtype=bool)
    assert not BR.phi_plane(e).any() and not BR.phi_plane(f).any()              # no boundary: phi = 0 (the full plane is the stated deviation)
    assert (BR.sq_transform(e) == -1).all()
    assert BR.surface(f).sum() == 2 * 4 + 2 * 6 - 4                              # the image border
    c, dab, dba = BR.surface_counters(e, f)
    assert c == [0, 16, -1, -1] and dab.size == 0
    assert all(math.isnan(v) for v in BR.surface_scores(e, f)) and all(math.isnan(v) for v in BR.surface_scores(e, e))
    # NaN and exactly the threshold are outside, the next float above it is inside
    y = np.array([[np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1.0))]], dtype=np.float32)
    assert BR.mask_of(y).tolist() == [[False, False, True]]


def test_the_boundary_term_by_hand_and_its_gradient():
    p = torch.tensor([[0.7, 0.3], [0.2, 0.8]], dtype=torch.float64)
    ph = torch.tensor([[0.0, 2.0], [1.0, -1.0]], dtype=torch.float64)
    lb = BR.boundary_term(p, ph, [0.0, 1.0], wb=0.5, ov_scale=0.5)
    assert abs(lb.item() - 0.5 * 0.5 / 2 * (0.3 * 2.0 - 0.8)) < 1e-16
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    cfg = R.config("dice", 2)
    r = BR.restate_at(p.float(), y, ph, cfg, [0.0, 1.0], 0.5, 1.0, 0.5)
    I, P, Y = R.sums(p.float().double(), y)
    A, B = R.coefficients(I, P, Y, cfg, 0.5)
    G = A * y + B + r["kb"] * torch.tensor([0.0, 1.0], dtype=torch.float64) * ph      # the header's summand wb*ov_scale*u_c*phi_c/M
    assert torch.allclose(r["G"], G, rtol=1e-13, atol=1e-18) and r["kb"] == 0.5 * 0.5 / 2
    r0 = BR.restate_at(p.float(), y, ph, cfg, [0.0, 1.0], 0.0, 1.0, 0.5)
    assert r0["lb"] == 0.0 and r0["loss"] == R.loss(p.float().double(), y, cfg, 1.0, 0.5).item()


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


NEW_SYMBOLS = ("usseg_sdf_ws_bytes", "usseg_sdf_labels", "usseg_surface_ws_bytes", "usseg_surface_dist", "usseg_overlap_boundary_loss_sums",
               "usseg_overlap_boundary_loss_bwd")


def test_exported_symbols_header_text_and_struct_layout():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "usseg.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in hdr, name
    assert C.sizeof(L.BoundaryLoss) == 32 and L.BoundaryLoss.u.offset == 0
    assert "typedef struct UssegBoundaryLoss {" in hdr and "float u[8];" in hdr
    assert C.sizeof(L.OverlapLoss) == 56                                          # pinned
    assert "#define USSEG_OVERLAP_ACC_FLOATS 8224 " in hdr
    for text in ("acc[12] = L_B alone", "acc[13] = wb*ov_scale/M", "covers the WHOLE image", "HD95", "binary_erosion(m, border_value=0)"):
        assert text in hdr, text
    from ultrasound_modeling_amd import ops
    assert ops.BOUNDARY_KEYS == ("weight", "class_weight", "threshold")
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    assert mk.count("sdf.hip") == 2                                               # built, and with the packed-fp32 flags off like its neighbours


def test_workspace_sizes():
    L, lib = _lib()
    assert lib.usseg_sdf_ws_bytes(16, 256, 80, 3) == 4 * 16 * 256 * 80 * 3 + 4 * 16 * 256
    assert lib.usseg_sdf_ws_bytes(1, 1, 9, 2) == 80 + 16                          # each region rounded up to 16 bytes
    assert lib.usseg_surface_ws_bytes(3, 5, 7) == 432
    for bad in ((1, 0, 8, 3), (1, 8, 0, 3), (1, 8193, 8, 3), (1, 8, 8193, 3), (1, 8, 8, 0), (1, 8, 8, 5), (-1, 8, 8, 3)):
        assert lib.usseg_sdf_ws_bytes(*bad) == -1, bad
    assert lib.usseg_sdf_ws_bytes(1, 8192, 8192, 4) == 4 * 8192 * 8192 * 4 + 4 * 8192
    assert lib.usseg_surface_ws_bytes(1, 0, 8) == -1 and lib.usseg_surface_ws_bytes(1, 8, 8193) == -1


def test_sdf_labels_refuses_bad_arguments_before_any_launch():
    """Non-null dummy pointers (16: aligned, never dereferenced): every case fails a check before the launch."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(y=16, B=1, H=8, W=8, C_=3, thr=0.5, phi=16, ws=16, ws_bytes=1 << 20):
        return lib.usseg_sdf_labels(y, B, H, W, C_, thr, phi, ws, ws_bytes, None)

    for kw in (dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(H=-3)):
        assert call(**kw) == -1 and "sdf_labels: H and W must lie in [1, 8192]" in err(), kw
    for c in (0, 5):
        assert call(C_=c) == -1 and "sdf_labels: 1 <= C <= 4" in err()
    for b in (-1, 65536):
        assert call(B=b) == -1 and "sdf_labels: 0 <= B <= 65535" in err()
    assert call(B=9, H=8192, W=8192, ws_bytes=1 << 40) == -1 and "more than 2^29 pixels" in err()
    assert call(thr=float("nan")) == -1 and "threshold is NaN" in err()
    for kw in (dict(y=None), dict(phi=None), dict(ws=None)):
        assert call(**kw) == -1 and "sdf_labels: null pointer" in err(), kw
    for kw in (dict(y=18), dict(phi=22), dict(ws=24)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    need = lib.usseg_sdf_ws_bytes(1, 8, 8, 3)
    assert call(ws_bytes=need - 1) == -1 and f"the workspace holds {need - 1} bytes, {need} needed" in err()
    assert call(B=0) == 0                                                         # nothing to do, nothing launched


def test_surface_dist_refuses_bad_arguments_before_any_launch():
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(a=16, b=16, N=1, H=8, W=8, counters=16, sums=16, ws=16, ws_bytes=1 << 20):
        return lib.usseg_surface_dist(a, b, N, H, W, counters, sums, ws, ws_bytes, None)

    for kw in (dict(H=0), dict(W=0), dict(H=8193), dict(W=8193)):
        assert call(**kw) == -1 and "surface_dist: H and W must lie in [1, 8192]" in err(), kw
    for n in (-1, 65536):
        assert call(N=n) == -1 and "surface_dist: 0 <= N <= 65535" in err()
    assert call(N=9, H=8192, W=8192, ws_bytes=1 << 40) == -1 and "more than 2^29 pixels" in err()
    for kw in (dict(a=None), dict(b=None), dict(counters=None), dict(sums=None), dict(ws=None)):
        assert call(**kw) == -1 and "surface_dist: null pointer" in err(), kw
    for kw in (dict(counters=20), dict(sums=12), dict(ws=8)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    assert call(ws_bytes=255) == -1 and "the workspace holds 255 bytes, 256 needed" in err()
    assert call(N=0) == 0


def _ol(L, **kw):
    cfg = dict(w=(0.2, 0.3, 0.5), alpha=0.5, beta=0.5, smooth=1.0, power=1.0, ov_weight=1.0, ce_weight=1.0)
    cfg.update(kw)
    w = list(cfg["w"]) + [0.0] * (8 - len(cfg["w"]))
    return L.OverlapLoss((C.c_float * 8)(*w), cfg["alpha"], cfg["beta"], cfg["smooth"], cfg["power"], cfg["ov_weight"], cfg["ce_weight"])


def _bl(L, u=(0.0, 1.0, 1.0)):
    return L.BoundaryLoss((C.c_float * 8)(*(list(u) + [0.0] * (8 - len(u)))))


def _desc(L, C_=3, M=32, HW=16, lddl=8, quad_w=0, eps=1e-7, ls=0.1, inv=0.25):
    return L.LossDesc(M, HW, C_, C_, lddl, 0, ls, eps, inv, quad_w)


@pytest.mark.parametrize("entry", ["overlap_boundary_loss_sums", "overlap_boundary_loss_bwd"])
def test_the_boundary_pair_refuses_bad_arguments_before_any_launch(entry):
    """Everything the plain pair refuses (tests/test_cpu_overlap_loss.py), under the new names, plus phi, the struct and wb."""
    L, lib = _lib()
    err = lambda: lib.usseg_last_error().decode()

    def call(d=None, ol=0, probs=16, y_true=16, phi=16, bl=0, wb=16, acc=16, acc_floats=8224, dl=16, ov_scale=1.0):
        d = C.byref(d) if d is not None else None
        ol = C.byref(_ol(L)) if ol == 0 else (None if ol is None else C.byref(ol))
        bl = C.byref(_bl(L)) if bl == 0 else (None if bl is None else C.byref(bl))
        if entry == "overlap_boundary_loss_sums":
            return lib.usseg_overlap_boundary_loss_sums(d, ol, ov_scale, probs, y_true, phi, bl, wb, acc, acc_floats, None)
        return lib.usseg_overlap_boundary_loss_bwd(d, ol, probs, y_true, phi, bl, acc, acc_floats, dl, None)

    assert call(d=None) == -1 and f"{entry}: null descriptor" in err()
    assert call(d=_desc(L), ol=None) == -1 and f"{entry}: null overlap-loss struct" in err()
    assert call(d=_desc(L), bl=None) == -1 and f"{entry}: null boundary-loss struct" in err()
    for kw in (dict(probs=None), dict(y_true=None), dict(acc=None), dict(phi=None)):
        assert call(d=_desc(L), **kw) == -1 and f"{entry}: null pointer" in err(), kw
    for bad_c in (0, 5):
        assert call(d=_desc(L, C_=bad_c)) == -1 and f"{entry}: 1 <= C <= 4" in err()
    for d in (_desc(L, M=33), _desc(L, HW=0), _desc(L, M=-16)):
        assert call(d=d) == -1 and "M must be a non-negative multiple of HW" in err()
    assert call(d=_desc(L, M=(1 << 29) + 16)) == -1 and "more than 2^29 pixels" in err()
    for kw in (dict(probs=20), dict(y_true=24), dict(phi=24)):
        assert call(d=_desc(L), **kw) == -1 and "aligned" in err(), kw
    for u in ((0.0, -1.0, 1.0), (0.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        assert call(d=_desc(L), bl=_bl(L, u)) == -1 and "boundary class weights must be finite and >= 0" in err(), u
    assert call(d=_desc(L), ol=_ol(L, smooth=0.0)) == -1 and "smooth must be finite and > 0" in err()
    assert call(d=_desc(L), ol=_ol(L, power=0.5)) == -1 and "power must lie in [1, 4]" in err()
    assert call(d=_desc(L), ol=_ol(L, w=(1.0, -0.5, 1.0))) == -1 and "class weights must be finite and >= 0" in err()
    assert call(d=_desc(L), acc_floats=31) == -1 and "header floats" in err()
    if entry == "overlap_boundary_loss_sums":
        assert call(d=_desc(L), wb=None) == -1 and f"{entry}: null pointer" in err()
        assert call(d=_desc(L), wb=18) == -1 and "aligned" in err()
        for s in (-1.0, float("nan"), float("inf")):
            assert call(d=_desc(L), ov_scale=s) == -1 and "ov_scale must be finite and >= 0" in err(), s
        assert call(d=_desc(L, M=2 * 256 * 80, HW=256 * 80), acc_floats=32 + 16 * 39) == -1 and "a grid of 40 workgroups needs 672 accumulator floats" in err()
    else:
        assert call(d=_desc(L), dl=None) == -1 and "dlogits must be a 16-byte aligned pointer" in err()
        assert call(d=_desc(L, lddl=16)) == -1 and "dlogits stride" in err()
        assert call(d=_desc(L, lddl=16, quad_w=3)) == -1 and "quad layout" in err()
        assert call(d=_desc(L, M=0)) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_losses_tuples_are_unchanged():
    from ultrasound_modeling_amd.VisionTransformer import LOSSES, OVERLAP_LOSSES
    assert LOSSES == ("cce", "my_loss_cat", "focal") and OVERLAP_LOSSES == ("dice", "tversky", "dice_ce")


def test_boundary_config_defaults_and_refusals():
    from ultrasound_modeling_amd import ops
    from ultrasound_modeling_amd.VisionTransformer import boundary_config
    w, bl, thr = boundary_config("dice", 3, {})
    assert (w, list(bl.u)[:3], thr) == (0.01, [0.0, 1.0, 1.0], 0.5)
    w, bl, thr = boundary_config("tversky", 2, dict(weight=0, class_weight=[0.5, 2.0], threshold=0.25))
    assert (w, list(bl.u)[:2], thr) == (0.0, [0.5, 2.0], 0.25)
    for loss, cfg in (("cce", {}), ("focal", {}), ("my_loss_cat", {}), ("dice", dict(wieght=1.0)), ("dice", dict(weight=-0.1)),
                      ("dice", dict(weight=float("nan"))), ("dice", dict(weight=float("inf"))), ("dice", dict(class_weight=[0.0, 1.0])),
                      ("dice", dict(class_weight=[0.0, 1.0, 1.0, 1.0])), ("dice", dict(class_weight=[0.0, -1.0, 1.0])),
                      ("dice", dict(threshold=float("nan"))), ("dice", 0.01)):
        with pytest.raises(ValueError):
            boundary_config(loss, 3, cfg)
    for u in ([], [1.0] * 5, [1.0, float("nan")]):
        with pytest.raises(ValueError):
            ops.boundary_loss(u)


def test_constructor_refusals_come_before_any_device_work():
    """Each of these raises ValueError from the argument checks at the top of the constructor, GPU or not."""
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for kw in (dict(loss="cce", boundary={}), dict(boundary={}), dict(loss="focal", boundary=dict(weight=0.1)), dict(loss="my_loss_cat", boundary={}),
               dict(loss="dice", overlap={}, boundary=dict(wieght=0.1)), dict(loss="dice", overlap={}, boundary=dict(weight=-1.0)),
               dict(loss="dice", overlap={}, boundary=dict(weight=float("inf"))), dict(loss="dice", overlap={}, boundary=dict(weight=float("nan"))),
               dict(loss="dice_ce", overlap={}, boundary=dict(class_weight=[0.0, 1.0])), dict(loss="tversky", overlap={}, boundary=dict(class_weight=[1.0] * 4))):
        with pytest.raises(ValueError):
            VisionTransformer(2, (64, 64), in_channels=1, **kw)
        with pytest.raises(ValueError):
            TransUNet((64, 64), batch_size=2, in_channels=1, **kw)
    for fn in (VisionTransformer.__init__, TransUNet.__init__):
        par = inspect.signature(fn).parameters
        assert par["boundary"].default is None and par["boundary"].kind is inspect.Parameter.KEYWORD_ONLY
        assert not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in par.values())


def test_the_drivers_signatures_and_the_command_line():
    from ultrasound_modeling_amd import MainNumpy, MainParallel, TBI_TransUNet
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main):
        par = inspect.signature(fn).parameters
        assert par["boundary"].default is None and par["boundary"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        assert par["loss"].default == "cce" and par["overlap"].default is None, fn
    for fn in (MainNumpy.Process.training, MainParallel.Process.training):
        par = inspect.signature(fn).parameters
        assert par["boundary_ramp"].default is None and par["boundary_ramp"].kind is inspect.Parameter.KEYWORD_ONLY, fn
    for loss in ("cce", "my_loss_cat", "focal"):
        with pytest.raises(SystemExit):
            MainParallel._cli(["a.npy", "b.npy", "--loss", loss, "--boundary-weight", "0.01"])
    with pytest.raises(SystemExit):
        MainParallel._cli(["a.npy", "b.npy", "--boundary-weight", "0.01"])
    with pytest.raises(SystemExit):
        MainParallel._cli(["a.npy", "b.npy", "--loss", "hinge"])                  # --loss keeps its six choices
    src = inspect.getsource(MainParallel._cli)
    assert 'choices=("cce", "my_loss_cat", "focal", "dice", "tversky", "dice_ce")' in src


def test_surface_scores_from_counters_and_the_evaluators_surface():
    from ultrasound_modeling_amd import TBIEvaluator
    from ultrasound_modeling_amd.metrics import surface_scores_from_counters
    s = surface_scores_from_counters(torch.tensor([[2, 4, 9, 16], [0, 3, -1, -1], [1, 1, 0, 0]]), torch.tensor([[5.0, 10.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64))
    assert s["hd"][0] == 4.0 and s["assd"][0] == 0.5 * (2.5 + 2.5) and math.isnan(s["hd"][1]) and math.isnan(s["assd"][1])
    assert s["hd"][2] == 0.0 and s["assd"][2] == 0.0 and s["n_a"].tolist() == [2, 0, 1] and s["n_b"].tolist() == [4, 3, 1]
    assert TBIEvaluator.PolarResult._fields == ("prob_map", "bleed_prob", "mask", "label", "bmode", "names")      # its six fields
    assert inspect.signature(TBIEvaluator.surface_scores).parameters["threshold"].default == 0.5
    assert "--surface-csv" in inspect.getsource(TBIEvaluator.main)
