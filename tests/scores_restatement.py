"""Restatement of include/usseg_scores.h (``usseg_image_confusion``, ``usseg_component_measure``, ``usseg_bootstrap_sums``) as plain loops over
pixels, components and draws with Python integers - written after the header's definitions, not after the kernels: no tiles, no waves, no
atomics.  Also the stand-ins the CPU tests put in place of the GPU wrappers of ``ops`` (they take and return CPU torch tensors), and the
synthetic evaluator result both test files score."""
import numpy as np
import torch

import components_restatement as CR

MASK64 = (1 << 64) - 1
EMPTY_MIN = 65536


# ---- the three definitions -----------------------------------------------------------------------------------------------------------------
def confusion(pred, truth, C, weight=None):
    """uint8 [N,H,W] class ids -> (cm int64 [N,C,C] with cm[n][truth][pred], wcm the same with each pixel counted weight[y][x] times or None,
    invalid int64 [N]: the pixels with an id >= C, counted in no cell)"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    N, H, W = pred.shape
    cm = [[[0] * C for _ in range(C)] for _ in range(N)]
    wcm = [[[0] * C for _ in range(C)] for _ in range(N)]
    invalid = [0] * N
    wl = None if weight is None else np.asarray(weight).astype(np.uint32).tolist()
    for n in range(N):
        pl, tl = pred[n].tolist(), truth[n].tolist()
        for y in range(H):
            for x in range(W):
                t, p = tl[y][x], pl[y][x]
                if t >= C or p >= C:
                    invalid[n] += 1
                    continue
                cm[n][t][p] += 1
                if wl is not None:
                    wcm[n][t][p] += wl[y][x]
    as64 = lambda v, shape: np.array(v, np.int64).reshape(shape)
    return as64(cm, (N, C, C)), (as64(wcm, (N, C, C)) if wl is not None else None), as64(invalid, (N,))


def measure(labels, wq, xq, yq, cap):
    """int32 [N,H,W] labels -> int64 [N,cap,8]: pixels, sum w, sum w*xq, sum w*yq, xq_min, xq_max, yq_min, yq_max of id k in row k-1; an absent
    id: zeros and the empty marker (65536, -1, 65536, -1); ids above cap skipped"""
    labels = np.asarray(labels)
    N, H, W = labels.shape
    wl, xl, yl = (np.asarray(t).astype(np.int64).tolist() for t in (wq, xq, yq))
    out = [[[0, 0, 0, 0, EMPTY_MIN, -1, EMPTY_MIN, -1] for _ in range(cap)] for _ in range(N)]
    for n in range(N):
        ll = labels[n].tolist()
        for y in range(H):
            for x in range(W):
                k = ll[y][x]
                if k < 1 or k > cap:
                    continue
                r, w, qx, qy = out[n][k - 1], wl[y][x], xl[y][x], yl[y][x]
                r[0] += 1
                r[1] += w
                r[2] += w * qx
                r[3] += w * qy
                r[4], r[5], r[6], r[7] = min(r[4], qx), max(r[5], qx), min(r[6], qy), max(r[7], qy)
    return np.array(out, np.int64).reshape(N, cap, 8)


def draw_index(seed, r, U, d):
    """draw d of replicate r over U units: the header's counter-based generator, modulo 2^64"""
    z = (seed + 0x9E3779B97F4A7C15 * (1 + r * U + d)) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return ((z >> 32) * U) >> 32


def bootstrap(rows, R, seed):
    """int64 [U,K] -> int64 [R,K]: replicate r = the sum of the U rows its draws name, in Python integers (asserted to fit int64)"""
    rows = np.asarray(rows, np.int64)
    U, K = rows.shape
    rl = rows.tolist()
    out = []
    for r in range(R):
        acc = [0] * K
        for d in range(U):
            src = rl[draw_index(seed, r, U, d)]
            for k in range(K):
                acc[k] += src[k]
        assert all(-(1 << 63) <= v < (1 << 63) for v in acc)
        out.append(acc)
    return np.array(out, np.int64).reshape(R, K)


# ---- stand-ins for the GPU wrappers (CPU tensors in, CPU tensors out) -----------------------------------------------------------------------
def ops_image_confusion(pred, truth, num_classes=2, weight=None, *, out=None):
    cm, wcm, inv = confusion(pred.numpy(), truth.numpy(), int(num_classes), None if weight is None else weight.numpy())
    return torch.from_numpy(cm), (torch.from_numpy(wcm) if wcm is not None else None), torch.from_numpy(inv)


def ops_component_measure(labels, weight, xq, yq, cap, *, out=None):
    return torch.from_numpy(measure(labels.numpy(), weight.numpy(), xq.numpy(), yq.numpy(), int(cap)))


def ops_bootstrap_sums(rows, replicates, seed=0, *, out=None, check=True):
    return torch.from_numpy(bootstrap(rows.numpy(), int(replicates), int(seed)))


def ops_label_components(mask, connectivity=8, labels=None, count=None, ws=None):
    lab, cnt = CR.label(mask.numpy(), connectivity)
    return torch.from_numpy(lab), torch.from_numpy(cnt)


def ops_component_overlap(la, lb, cap_a, cap_b):
    ha, hb = CR.overlap(la.numpy(), lb.numpy(), int(cap_a), int(cap_b))
    return torch.from_numpy(ha), torch.from_numpy(hb)


def ops_component_stats(labels, cap, prob=None):
    return torch.from_numpy(CR.stats(labels.numpy(), int(cap), None if prob is None else prob.numpy()))


def ops_clean_mask(mask, prob=None, *, connectivity=8, min_area=1, min_peak=0.0, out=None, ws=None):
    return torch.from_numpy(CR.clean(mask.numpy(), None if prob is None else prob.numpy(), connectivity, min_area, min_peak))


STAND_INS = {"image_confusion": ops_image_confusion, "component_measure": ops_component_measure, "bootstrap_sums": ops_bootstrap_sums,
             "label_components": ops_label_components, "component_overlap": ops_component_overlap, "component_stats": ops_component_stats,
             "clean_mask": ops_clean_mask}


# ---- the shapes and the synthetic run both test files use -------------------------------------------------------------------------------------
def polar_axes(H, W, r0=20.0, dr=0.25, t0=-0.5, dt=0.0125):
    """a sector scan: x = r sin(theta), y = r cos(theta), r = r0 + i*dr down the rows, theta = t0 + j*dt along the columns"""
    r = r0 + dr * np.arange(H, dtype=np.float64)[:, None]
    th = t0 + dt * np.arange(W, dtype=np.float64)[None, :]
    return r * np.sin(th), r * np.cos(th)


def synthetic_result(E, N=6, H=24, W=20, seed=3):
    """A ``TBIEvaluator.PolarResult`` of N images in N // 2 "patients" (DoD001, DoD001, DoD002, ...): labelled discs, a prediction that is the
    label shifted by a pixel plus speckle; image 1 is empty in both masks (its Dice is undefined), image 2 has a label and no prediction."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    label = np.zeros((N, H, W), np.float32)
    prob = np.zeros((N, H, W), np.float32)
    for n in range(N):
        if n == 1:
            continue
        cy, cx, r = rng.integers(6, H - 6), rng.integers(6, W - 6), rng.integers(2, 5)
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        label[n] = np.where(disc, 2.0, 1.0)
        if n == 2:
            continue
        shifted = np.roll(disc, (1, -1), (0, 1))
        prob[n] = np.where(shifted, 0.9, 0.1) + np.where(rng.random((H, W)) < 0.02, 0.5, 0.0)
    prob = np.clip(prob, 0.0, 1.0).astype(np.float32)
    names = np.array([f"DoD{n // 2 + 1:03d}_frame{n}" for n in range(N)])
    return E.PolarResult(prob_map=prob.copy(), bleed_prob=prob, mask=np.ones((N, H, W), np.float32), label=label, bmode=np.zeros((N, H, W), np.float32),
                         names=names)
