"""CPU tests of the evaluator's cone figures (TBIEvaluator.ConeGeometry / render_figures / Display): known answers of the index rule of
tests/cone_restatement.py on hand-built grids, its agreement with matplotlib's Agg pcolormesh on the synthetic fan, the colour rule
against Normalize + Colormap(bytes=True), the bMode range against np.histogram, the PNG writer decoded by PIL, and the argument
checks, all without a launch."""
import numpy as np
import pytest
import torch

import cone_restatement as R


def _grid(*rows):
    """X, Y [H,W] from rows of (x, y) vertices."""
    a = np.array(rows, np.float64)
    return np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1])


# ------------------------------------------------------------------------------------------------ the index rule
def test_unit_squares_and_background():
    # two unit squares side by side at 2 px per unit, the top-right unit left empty by a third row that folds back
    X, Y = _grid([(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (2, 1)])
    idx = R.cone_index(X, Y, 2)
    np.testing.assert_array_equal(idx, [[0, 0, 1, 1], [0, 0, 1, 1]])
    X, Y = _grid([(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (1, 0)])   # quad 1 is the zero-area segment (1,0)-(2,0)-(1,0)-(1,1)
    idx = R.cone_index(X, Y, 2)
    np.testing.assert_array_equal(idx, [[0, 0, -1, -1], [0, 0, -1, -1]])


def test_later_quad_overwrites_earlier():
    # quad 0 covers [0,2]x[0,1]; quad 1 folds back over its right half
    X, Y = _grid([(0, 0), (2, 0), (1, 0)], [(0, 1), (2, 1), (1, 1)])
    np.testing.assert_array_equal(R.cone_index(X, Y, 2), [[0, 0, 1, 1], [0, 0, 1, 1]])


def test_zero_area_quad_covers_nothing():
    X, Y = _grid([(0, 0), (3, 0)], [(0, 0), (3, 0)])          # all four vertices on one line: Hp = 0
    assert R.layout(X, Y, 2)[2] == 0
    X, Y = _grid([(0, 0), (2, 2)], [(1, 1), (1, 1)])          # a degenerate quad inside a non-empty box
    idx = R.cone_index(X, Y, 2)
    assert idx.shape == (4, 4) and (idx == -1).all()


def test_bow_tie_under_nonzero_winding():
    # vertices (0,0) -> (2,2) -> (2,0) -> (0,2): two lobes of opposite orientation, winding +1 and -1, both covered
    X, Y = _grid([(0, 0), (2, 2)], [(0, 2), (2, 0)])
    assert R.winding((0, 2, 2, 0), (0, 2, 0, 2), np.array([0.5, 1.5]), np.array([1.0, 1.0])).tolist() == [1, -1]
    idx = R.cone_index(X, Y, 2)       # centres at 0.25, 0.75, 1.25, 1.75: the left lobe is x < min(y, 2-y), the right x > max(y, 2-y)
    assert (idx[1:3, 0] == 0).all() and (idx[1:3, 3] == 0).all()          # inside the left (+1) and the right (-1) lobe
    assert (idx[[0, 0, 3, 3], [1, 2, 1, 2]] == -1).all()                  # above and below the crossing
    # centres on the diagonals go by the half-open rule: exactly one of two mirrored points, never both
    np.testing.assert_array_equal(idx, [[-1, -1, -1, 0], [0, -1, 0, 0], [0, -1, 0, 0], [-1, -1, -1, 0]])


def test_sample_on_an_edge_takes_the_half_open_side():
    # quad 0 spans y in [1,2], quad 1 (drawn later) y in [0,1]; at 0.5 px per unit the single sample row sits exactly on y = 1.
    # y0 <= py < y1 gives the shared edge to the quad above it (quad 0), although quad 1 is drawn later.
    X, Y = _grid([(0, 2), (4, 2)], [(0, 1), (4, 1)], [(0, 0), (4, 0)])
    assert R.layout(X, Y, 0.5) == (0.0, 0.0, 1, 2)
    np.testing.assert_array_equal(R.cone_index(X, Y, 0.5), [[0, 0]])
    # the same on a vertical edge: the sample x = 1 belongs to the quad on its right, whichever is drawn later
    X, Y = _grid([(1, 0), (2, 0)], [(1, 2), (2, 2)])
    X2, Y2 = _grid([(1, 0), (0, 0)], [(1, 2), (0, 2)])       # the same square [0,1] x [0,2] drawn from the right: quad 0 = [0,1]
    Xa, Ya = np.hstack([X2[:, ::-1], X[:, 1:]]), np.hstack([Y2[:, ::-1], Y[:, 1:]])   # columns x = 0, 1, 2: quads [0,1] and [1,2]
    np.testing.assert_array_equal(R.cone_index(Xa, Ya, 0.5), [[1]])
    np.testing.assert_array_equal(R.cone_index(Xa[:, ::-1], Ya[:, ::-1], 0.5), [[0]])    # mirrored order: the right quad is 0


def test_fan_layout():
    X, Y = R.fan()
    assert X.shape == (256, 80) and (X == np.round(X)).all()
    xmin, ymin, Hp, Wp = R.layout(X, Y, 2)
    assert (xmin, ymin) == (3.0, 0.0) and (Hp, Wp) == (290, 386)


# ------------------------------------------------------------------------------------------------ against matplotlib
def test_index_agrees_with_agg_pcolormesh_within_one_pixel():
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    X, Y = R.fan()
    ppu = 2
    _, _, Hp, Wp = R.layout(X, Y, ppu)
    C = np.random.default_rng(0).uniform(0, 2, X.shape)
    dpi = 100
    fig = plt.figure(figsize=(Wp / dpi, Hp / dpi), dpi=dpi, facecolor="white")
    try:
        ax = fig.add_axes([0, 0, 1, 1])
        ax.set_axis_off()
        ax.pcolormesh(X, Y, C[:-1, :-1], shading="flat", cmap="magma", vmin=0, vmax=2)
        ax.set_xlim(X.min(), X.max())
        ax.set_ylim(Y.max(), Y.min())
        fig.canvas.draw()
        agg = np.asarray(fig.canvas.buffer_rgba())[..., :3].copy()
    finally:
        plt.close(fig)
    assert agg.shape == (Hp, Wp, 3)
    # Agg fills with the colour rounded to 8 bits; the product's bytes=True table truncates (a deviation of at most 1 per channel)
    rounded = np.floor(matplotlib.colormaps["magma"](range(256))[:, :3] * 255 + 0.5).astype(np.uint8)
    assert np.abs(rounded.astype(int) - R.luts()[0]).max() <= 1
    mine = R.colourise(R.cone_index(X, Y, ppu), C, 0.0, 2.0, rounded)
    pad = np.pad(mine, ((1, 1), (1, 1), (0, 0)), constant_values=255)
    near = np.zeros((Hp, Wp), bool)
    for dr in range(3):
        for dc in range(3):
            near |= (pad[dr:dr + Hp, dc:dc + Wp] == agg).all(-1)
    assert near.mean() >= 0.995, f"{(~near).sum()} of {near.size} pixels have no matching colour within one pixel"
    assert 0.85 < (mine == agg).all(-1).mean() < 1.0        # Agg's coverage fill of the slivers is not the centre rule: not exact


def test_colour_rule_matches_normalize_and_colormap():
    import matplotlib
    from matplotlib.colors import Normalize
    magma = R.luts()[0]
    rng = np.random.default_rng(1)
    # values away from the bin boundaries k/256 (the product works in fp64, matplotlib in the data's dtype)
    k = rng.integers(0, 256, 4000)
    v = (k + rng.uniform(0.05, 0.95, k.size)) / 256 * 2.0
    v = np.concatenate([v, [-1.0, -1e-9, 0.0, 2.0, 2.5, 1e300, np.nan, np.inf, -np.inf]])
    ref = matplotlib.colormaps["magma"](Normalize(0.0, 2.0)(np.ma.masked_invalid(v)), bytes=True)
    got_k, valid = R.colour_index(v, 0.0, 2.0)
    np.testing.assert_array_equal(valid, ref[:, 3] == 255)
    np.testing.assert_array_equal(magma[got_k[valid]], ref[valid, :3])
    assert (ref[~valid, 3] == 0).all() and (~valid).sum() == 3              # pcolormesh masks NaN and both infinities
    # vmin == vmax: Normalize maps every value to 0
    got_k, valid = R.colour_index(np.array([-3.0, 0.5, 0.5, 7.0, np.nan]), 0.5, 0.5)
    ref = matplotlib.colormaps["magma"](Normalize(0.5, 0.5)(np.ma.masked_invalid([-3.0, 0.5, 0.5, 7.0, np.nan])), bytes=True)
    np.testing.assert_array_equal(got_k[:4], [0, 0, 0, 0])
    np.testing.assert_array_equal(magma[got_k[:4]], ref[:4, :3])
    assert not valid[4]


def test_histogram_edges_formula_is_bit_equal():
    rng = np.random.default_rng(2)
    cases = [rng.standard_normal((256, 80)) * 30 - 5, -np.abs(rng.standard_normal((256, 80))) * 1e-3, np.full((256, 80), -2.75),
             np.zeros((256, 80)), rng.integers(-9, 9, (256, 80)).astype(np.float64), np.array([[1e-300, 3e-300]])]
    for b in cases:
        first, last = b.min(), b.max()
        if first == last:
            first, last = first - 0.5, last + 0.5
        delta = last - first
        step = delta / 25.0
        e = (2.0 * step + first, 24.0 * step + first) if step != 0 else ((2.0 / 25.0) * delta + first, (24.0 / 25.0) * delta + first)
        assert np.array(e).view(np.int64).tolist() == np.array(R.bmode_range(b)).view(np.int64).tolist()
    for bad in ([[0.0, np.nan]], [[0.0, np.inf]], [[0.0, 5e-324]], [[1.0, np.nextafter(1.0, 2.0)]]):   # non-finite; too narrow for 25 bins
        with pytest.raises(ValueError):
            R.bmode_range(np.array(bad))


# ------------------------------------------------------------------------------------------------ PNG writer
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (290 * 2 + 16, 386 * 2 + 16)])
def test_png_writer_round_trip(tmp_path, shape):
    from PIL import Image
    from ultrasound_modeling_amd.TBIEvaluator import write_png
    rgb = np.random.default_rng(3).integers(0, 256, shape + (3,), dtype=np.uint8)
    rgb[: shape[0] // 2] = 255
    path = str(tmp_path / "a.png")
    write_png(path, rgb)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (shape[1], shape[0])
        np.testing.assert_array_equal(np.asarray(im), rgb)


def test_png_writer_refuses_bad_arrays(tmp_path):
    from ultrasound_modeling_amd.TBIEvaluator import write_png
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "b.png"), bad)


# ------------------------------------------------------------------------------------------------ refusals without a launch
def test_geometry_refusals():
    from ultrasound_modeling_amd.TBIEvaluator import ConeGeometry
    X, Y = R.fan(int_axes=False)
    bad = [
        dict(xAxis=X, yAxis=Y[:, :-1]),                          # shapes differ
        dict(xAxis=X[:1], yAxis=Y[:1]),                          # one row of vertices: no quad
        dict(xAxis=X.ravel(), yAxis=Y.ravel()),                  # not a grid
        dict(xAxis=np.where(X > 150, np.nan, X), yAxis=Y),       # non-finite vertices
        dict(xAxis=X, yAxis=Y, px_per_unit=0),
        dict(xAxis=X, yAxis=Y, px_per_unit=-2),
        dict(xAxis=X, yAxis=Y, px_per_unit=float("inf")),
        dict(xAxis=X, yAxis=Y, px_per_unit=400),                 # a 58k x 77k panel: int32 byte offsets overflow
        dict(xAxis=np.zeros((4, 4)), yAxis=np.zeros((4, 4))),   # no area
        dict(xAxis=X, yAxis=Y, gap=-1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ConeGeometry(device="cpu", **kw)


def test_op_wrappers_refuse_before_launch():
    from ultrasound_modeling_amd import ops
    X = torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.cone_index(X, X, 0.0, 0.0, 2.0, 4, 4)                                     # host tensors
    with pytest.raises(ValueError):
        ops.cone_range(torch.zeros(2, 4, 4, dtype=torch.float32))
    p32, p64 = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.cone_render(torch.zeros(3, 3, dtype=torch.int32), p32, p64, p32, p64, ((0, 2),) * 3, torch.zeros(2, 2, dtype=torch.float64),
                        torch.zeros(2, 256, 3, dtype=torch.uint8), 4)


def test_display_refuses_bad_names_and_batches(tmp_path):
    from ultrasound_modeling_amd.TBIEvaluator import Display, PolarResult, render_figures
    z = np.zeros((2, 256, 80))
    res = PolarResult(z.astype(np.float32), z.astype(np.float32), None, z, z, np.array(["ok", "a/b"]))
    with pytest.raises(ValueError, match="'/'"):
        Display(res, None, str(tmp_path))
    with pytest.raises(ValueError):
        Display(res._replace(names=np.array(["x"])), None, str(tmp_path))              # one name for two images
    assert not any(tmp_path.iterdir())

    class Geo:          # the attributes render_figures reads before it launches
        grid, figure_shape = (256, 80), (8, 8, 3)
    for bad in (res._replace(names=None, label=z[:, :, :40]), ):
        with pytest.raises(ValueError):
            render_figures(bad, Geo())
    with pytest.raises(ValueError):
        render_figures(res._replace(names=None), Geo(), batch_size=0)
    g = Geo()
    g.grid = (256, 81)
    with pytest.raises(ValueError, match="vertex grid"):
        render_figures(res._replace(names=None), g)


def test_cli_help_and_import_touch_nothing(tmp_path):
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "ultrasound_modeling_amd.TBIEvaluator", "--help"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--bleed" in r.stdout and "--px-per-unit" in r.stdout and "--no-stamp" in r.stdout
    assert not any(tmp_path.iterdir())
