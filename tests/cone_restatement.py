"""A float64 NumPy restatement of the evaluator's cone figures (TBIEvaluator.Display of the reference: four pcolormesh panels per image),
written from the rules of DESIGN.md section 4i - not from the kernels - plus the synthetic fan geometry the tests draw on.

  index:  pixel (r, c) samples (xmin + (c+0.5)/ppu, ymin + (r+0.5)/ppu) and shows the largest row-major quad q = i*(W-1) + j, vertices
          (i,j), (i,j+1), (i+1,j+1), (i+1,j), whose nonzero winding number there is not 0; half-open crossings: an upward edge
          (y0 <= py < y1) with isLeft > 0 counts +1, a downward edge (y1 <= py < y0) with isLeft < 0 counts -1,
          isLeft = (x1-x0)*(py-y0) - (px-x0)*(y1-y0).  -1 where no quad covers the pixel.
  colour: t = (v - vmin)/(vmax - vmin), k = clamp(floor(t*256), 0, 255), k = 0 when vmax == vmin; NaN / inf -> white.
  bMode:  vmin, vmax = np.histogram(bMode, bins=25)[1][[2, -2]].
"""
import numpy as np

WHITE = np.array([255, 255, 255], np.uint8)


def fan(H=256, W=80, r=(5.0, 150.0), theta=0.7, int_axes=True):
    """The synthetic scan geometry: depth r down the rows, angle across the columns; x = r sin(theta) + 100, y = r cos(theta) - 4."""
    rr = np.linspace(r[0], r[1], H)[:, None]
    th = np.linspace(-theta, theta, W)[None, :]
    X = rr * np.sin(th) + 100
    Y = rr * np.cos(th) - 4
    if int_axes:
        X, Y = X.astype(int), Y.astype(int)
    return X.astype(np.float64), Y.astype(np.float64)


def layout(X, Y, ppu):
    """-> (xmin, ymin, Hp, Wp)."""
    xmin, xmax, ymin, ymax = X.min(), X.max(), Y.min(), Y.max()
    return float(xmin), float(ymin), int(np.ceil((ymax - ymin) * ppu)), int(np.ceil((xmax - xmin) * ppu))


def winding(vx, vy, px, py):
    """Nonzero winding number of the closed polygon (vx, vy) at the points (px, py), half-open crossing rule."""
    wn = np.zeros(np.broadcast(px, py).shape, np.int32)
    n = len(vx)
    for e in range(n):
        x0, y0, x1, y1 = vx[e], vy[e], vx[(e + 1) % n], vy[(e + 1) % n]
        il = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
        wn += ((y0 <= py) & (py < y1) & (il > 0)).astype(np.int32)
        wn -= ((y1 <= py) & (py < y0) & (il < 0)).astype(np.int32)
    return wn


def cone_index(X, Y, ppu):
    """int32 [Hp,Wp]: the quad each pixel centre shows (draw order: the last quad wins), -1 for background."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    H, W = X.shape
    xmin, ymin, Hp, Wp = layout(X, Y, ppu)
    px = xmin + (np.arange(Wp) + 0.5) / ppu
    py = ymin + (np.arange(Hp) + 0.5) / ppu
    out = np.full((Hp, Wp), -1, np.int32)
    for i in range(H - 1):
        for j in range(W - 1):
            vx = (X[i, j], X[i, j + 1], X[i + 1, j + 1], X[i + 1, j])
            vy = (Y[i, j], Y[i, j + 1], Y[i + 1, j + 1], Y[i + 1, j])
            # pixels whose centre lies in the quad's bounding box (the winding test decides; a box only limits the work)
            c = np.nonzero((px >= min(vx)) & (px <= max(vx)))[0]
            r = np.nonzero((py >= min(vy)) & (py <= max(vy)))[0]
            if len(c) == 0 or len(r) == 0:
                continue
            hit = winding(vx, vy, px[c][None, :], py[r][:, None]) != 0
            sub = out[np.ix_(r, c)]
            sub[hit] = i * (W - 1) + j            # row-major order: every later quad overwrites
            out[np.ix_(r, c)] = sub
    return out


def colour_index(v, vmin, vmax):
    """-> (k int [..], valid bool [..]): the colormap entry of each value and whether it is finite (drawn at all)."""
    v = np.asarray(v, np.float64)
    valid = np.isfinite(v)
    if vmax == vmin:
        return np.zeros(v.shape, np.int64), valid
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((v - vmin) / (vmax - vmin) * 256.0)
    k = np.where(f >= 255, 255, np.where(f >= 0, f, 0))
    return np.where(valid, k, 0).astype(np.int64), valid


def bmode_range(bmode):
    """np.histogram's edges [2] and [-2] (raises on non-finite values, as the reference's call does)."""
    e = np.histogram(np.asarray(bmode, np.float64), bins=25)[1]
    return float(e[2]), float(e[-2])


def colourise(index, values, vmin, vmax, lut):
    """One panel: uint8 [Hp,Wp,3] of the quad values values[i, j] (the trimmed C[:-1, :-1]) through lut [256,3]."""
    H, W = values.shape
    out = np.empty(index.shape + (3,), np.uint8)
    out[:] = WHITE
    q = index[index >= 0]
    k, valid = colour_index(np.asarray(values, np.float64)[q // (W - 1), q % (W - 1)], vmin, vmax)
    rgb = lut[k]
    rgb[~valid] = WHITE
    out[index >= 0] = rgb
    return out


def figure(index, prob_map, label, bleed_prob, bmode, magma, binary, gap):
    """One image's figure: uint8 [2*Hp+gap, 2*Wp+gap, 3], panels Prediction | label / Probability Bleed | bMode on white."""
    Hp, Wp = index.shape
    out = np.empty((2 * Hp + gap, 2 * Wp + gap, 3), np.uint8)
    out[:] = WHITE
    lo, hi = bmode_range(bmode)
    panels = ((prob_map, 0.0, 2.0, magma), (label, 0.0, 2.0, magma), (bleed_prob, 0.0, 1.0, magma), (bmode, lo, hi, binary))
    for p, (v, a, b, lut) in enumerate(panels):
        r0, c0 = (p // 2) * (Hp + gap), (p % 2) * (Wp + gap)
        out[r0:r0 + Hp, c0:c0 + Wp] = colourise(index, v, a, b, lut)
    return out


def luts():
    """(magma, binary) uint8 [256,3] from matplotlib, as the product builds them."""
    import matplotlib
    return tuple(np.asarray(matplotlib.colormaps[n](range(256), bytes=True))[:, :3].copy() for n in ("magma", "binary"))
