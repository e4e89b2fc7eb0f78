"""NumPy restatement of the connected-component definitions of include/usseg.h (``usseg_label_components``, ``usseg_component_stats``,
``usseg_clean_mask``, ``usseg_component_overlap``) and of the lesion scores of ``metrics.lesion_scores_from_tables`` - written after the
definitions, not after the kernels: a plain flood fill in raster order, Python loops over components, no union-find."""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label_plane(mask, connectivity=8):
    """[H,W] -> (labels int32 [H,W], K): the pixels are visited in raster order; an unlabelled mask pixel opens the next id and floods it."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    lab = np.zeros((H, W), np.int32)
    k = 0
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or lab[y0, x0]:
                continue
            k += 1
            lab[y0, x0] = k
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in NEIGHBOURS[connectivity]:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = k
                        stack.append((yy, xx))
    return lab, k


def label(mask, connectivity=8):
    """[N,H,W] -> (labels int32 [N,H,W], count int32 [N])"""
    planes = [label_plane(p, connectivity) for p in np.asarray(mask)]
    N = len(planes)
    labels = np.stack([p[0] for p in planes]) if N else np.zeros(np.shape(mask), np.int32)
    return labels, np.array([p[1] for p in planes], np.int32)


def peak_bits(values):
    """the fp32 bit pattern of the largest value that is not NaN (and above 0), widened; 0 when there is none"""
    v = np.asarray(values, np.float32)
    v = v[~np.isnan(v)]
    v = v[v > 0]
    return int(np.float32(v.max()).view(np.uint32)) if v.size else 0


def stats(labels, cap, prob=None):
    """int64 [N,cap,8]: area, y_min, x_min, y_max, x_max, sum y, sum x, peak bits; rows of absent ids zero, ids above cap skipped"""
    labels = np.asarray(labels)
    N = labels.shape[0]
    out = np.zeros((N, cap, 8), np.int64)
    for n in range(N):
        for k in range(1, min(cap, int(labels[n].max(initial=0))) + 1):
            ys, xs = np.nonzero(labels[n] == k)
            if ys.size == 0:
                continue
            out[n, k - 1] = [ys.size, ys.min(), xs.min(), ys.max(), xs.max(), ys.sum(), xs.sum(),
                             peak_bits(prob[n][ys, xs]) if prob is not None else 0]
    return out


def clean(mask, prob=None, connectivity=8, min_area=1, min_peak=0.0):
    """uint8 [N,H,W]: 1 on the components with area >= min_area and, with prob, a peak >= min_peak"""
    labels, count = label(mask, connectivity)
    out = np.zeros(labels.shape, np.uint8)
    for n in range(labels.shape[0]):
        for k in range(1, int(count[n]) + 1):
            sel = labels[n] == k
            ok = int(sel.sum()) >= min_area
            if prob is not None:
                ok = ok and np.uint32(peak_bits(prob[n][sel])).view(np.float32) >= np.float32(min_peak)      # (the C ABI takes min_peak as fp32)
            if ok:
                out[n][sel] = 1
    return out


def overlap(la, lb, cap_a, cap_b):
    """(hit_a int32 [N,cap_a], hit_b int32 [N,cap_b]): pixels of each component inside any component of the other image"""
    la, lb = np.asarray(la), np.asarray(lb)
    N = la.shape[0]
    ha, hb = np.zeros((N, cap_a), np.int32), np.zeros((N, cap_b), np.int32)
    for n in range(N):
        for k in range(1, cap_a + 1):
            ha[n, k - 1] = int(((la[n] == k) & (lb[n] > 0)).sum())
        for k in range(1, cap_b + 1):
            hb[n, k - 1] = int(((lb[n] == k) & (la[n] > 0)).sum())
    return ha, hb


def div_no_nan(a, b):
    return a / b if b != 0 else 0.0


def lesion_scores(pred, true, connectivity=8, min_overlap=1):
    """The definitions, image by image: a labelled lesion is detected if at least min_overlap of its pixels lie inside the prediction; a
    predicted component is a false positive if none of its pixels lies inside the label."""
    pred, true = np.asarray(pred) != 0, np.asarray(true) != 0
    N = pred.shape[0]
    rows = {k: [] for k in ("n_true", "n_pred", "detected", "missed", "false_pos", "largest_true", "largest_pred")}
    for n in range(N):
        lt, kt = label_plane(true[n], connectivity)
        lp, kp = label_plane(pred[n], connectivity)
        det = sum(1 for k in range(1, kt + 1) if int(((lt == k) & pred[n]).sum()) >= min_overlap)
        fp = sum(1 for k in range(1, kp + 1) if not ((lp == k) & true[n]).any())
        rows["n_true"].append(kt)
        rows["n_pred"].append(kp)
        rows["detected"].append(det)
        rows["missed"].append(kt - det)
        rows["false_pos"].append(fp)
        rows["largest_true"].append(max([int((lt == k).sum()) for k in range(1, kt + 1)], default=0))
        rows["largest_pred"].append(max([int((lp == k).sum()) for k in range(1, kp + 1)], default=0))
    out = {k: np.array(v, np.int64) for k, v in rows.items()}
    sens = div_no_nan(float(out["detected"].sum()), float(out["n_true"].sum()))
    prec = div_no_nan(float(out["n_pred"].sum() - out["false_pos"].sum()), float(out["n_pred"].sum()))
    out.update(sensitivity=sens, precision=prec, f1=div_no_nan(2.0 * prec * sens, prec + sens), fp_per_image=div_no_nan(float(out["false_pos"].sum()), float(N)))
    return out


# ---- the shapes both test files label -----------------------------------------------------------------------------------------------------
def spiral(n=33):
    """one-pixel-wide rectangular spiral in an n x n plane, one free pixel between its turns: one component with the longest chain of parents"""
    m = np.zeros((n, n), np.uint8)
    inside = lambda y, x: 0 <= y < n and 0 <= x < n
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    for _ in range(n * n):
        for _turn in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            ok = inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax])
            if ok:
                break
            dy, dx = dx, -dy                                    # right -> down -> left -> up
        if not ok:
            break
        y, x = ny, nx
        m[y, x] = 1
    return m[None]


def comb(H=40, W=131):
    """a full top row with every second column hanging from it: many provisional labels that merge late"""
    m = np.zeros((1, H, W), np.uint8)
    m[0, :, ::2] = 1
    m[0, 0, :] = 0
    m[0, H - 1, :] = 1                    # the joining row comes LAST in raster order, and a second comb hangs from a top row
    m = np.concatenate([m, m[:, ::-1]])
    return np.ascontiguousarray(m)


def checkerboard(n=16):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((yy + xx) % 2 == 0).astype(np.uint8)[None]


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def blobs_and_speckle(N=16, H=256, W=80, seed=5):
    """the evaluator's shape: one or two discs per image plus 1 % single-pixel speckle"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = rng.random((N, H, W)) < 0.01
    for n in range(N):
        for _ in range(1 + n % 2):
            cy, cx, r = rng.integers(10, H - 10), rng.integers(10, W - 10), rng.integers(3, 12)
            m[n] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def label_cases():
    """name -> uint8 [N,H,W]: the smallest shapes at which each part of a labelling kernel can go wrong"""
    mixed = np.stack([np.zeros((21, 70), np.uint8), random_mask((21, 70), 0.5, 11), np.ones((21, 70), np.uint8), random_mask((21, 70), 0.5, 12),
                      np.zeros((21, 70), np.uint8)])
    line = random_mask((1, 1, 130), 0.6, 2)
    line[0, 0, 60:70] = 1                                       # a run across the 64-pixel word boundary
    return {
        "2x1x1": np.array([[[1]], [[0]]], np.uint8),
        "1x1x130": line,
        "1x130x1": np.ascontiguousarray(line.transpose(0, 2, 1)),
        "3x5x7": random_mask((3, 5, 7), 0.5, 3),
        "2x67x129 d0.41": random_mask((2, 67, 129), 0.41, 4),
        "2x67x129 d0.59": random_mask((2, 67, 129), 0.59, 5),
        "spiral 33": spiral(33),
        "comb": comb(),
        "checkerboard 16": checkerboard(16),
        "empty, random, full": mixed,
        "2x300x300 d0.6": random_mask((2, 300, 300), 0.6, 6),
        "16x256x80 blobs + speckle": blobs_and_speckle(),
    }
