"""DataFilePlayGround's dataAug and oversampling block on the GPU (csrc/prep_aug.hip) against the NumPy restatement of
tests/prepaug_restatement.py: the exact order statistics against np.sort, each step alone and the whole chain (bit for bit except the
rotation, which is bounded per channel plane by the restatement's own fp64-vs-longdouble error), per-sample masking, determinism, the
generated noise, and build_arrays(oversample="bleed") end to end on a synthetic patient tree.

Rotation bound per plane: 8 * max|restatement_fp64 - restatement_longdouble|, floor 2^-50 * max|plane|."""
import os
import random

import numpy as np
import pytest
import torch

import prep_restatement as PR
import prepaug_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(a):
    return a.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------ exact order statistics
def _select_inputs(n, rng):
    low8 = np.float64(1.2345).view(np.uint64) & ~np.uint64(255)
    mixed = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    mixed[rng.uniform(size=n) < 0.2] = -0.0
    mixed[rng.uniform(size=n) < 0.1] = 0.0
    return {
        "all_equal": np.full(n, -3.25),
        "zeros95": np.where(rng.uniform(size=n) < 0.95, 0.0, rng.standard_normal(n)),
        "low8": (low8 | rng.integers(0, 256, n).astype(np.uint64)).view(np.float64),
        "mixed": mixed,
    }


@pytest.mark.parametrize("n", [1000, 1531, 245760])
def test_select_ranks_against_sort(n):
    from ultrasound_modeling_amd import ops
    rng = np.random.default_rng(n)
    N = 1 if n == 245760 else 3
    k = n // 50
    for ranks in ([0, n - 1, k, k + 1], [n - 2, n - 1], [n // 2]):
        for name, x in _select_inputs(N * n, rng).items():
            x = x.reshape(N, n)
            got = ops.select_ranks_f64(torch.from_numpy(x).to(DEV), ranks).cpu().numpy()
            ref = np.sort(x, axis=1)[:, ranks]
            assert (got == ref).all(), (name, ranks, got, ref)
            assert not np.signbit(got[got == 0]).any()
    x = torch.from_numpy(_select_inputs(N * n, rng)["mixed"].reshape(N, n)).to(DEV)
    a, b = ops.select_ranks_f64(x, [0, k, k + 1, n - 1]), ops.select_ranks_f64(x, [0, k, k + 1, n - 1])
    assert torch.equal(_bits(a), _bits(b))
    if N == 3:                                                             # a masked segment is left alone
        act = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
        m = ops.select_ranks_f64(x, [k], act).cpu().numpy()
        assert np.isnan(m[1, 0]) and m[0, 0] == a[0, 1].item() and m[2, 0] == a[2, 1].item()


# ------------------------------------------------------------------------------------------------ the steps and the chain
SHAPES = {"small": (3, 24, 20, 12), "odd": (2, 37, 19, 5), "full": (4, 256, 80, 12)}


def _param_sets(H, W):
    box = (H // 2, W // 2, max(2, H // 5), max(2, W // 5))
    edge = (H - 1, W - 1, 3, 3)                                            # reaches the last row / column, which the loops never touch
    sr, sc = min(30, H // 3), min(12, W // 3)
    P = R.params
    return [
        P(), P(flip=True), P(reduc=True), P(contrast=True), P(clip=box), P(clip=edge), P(rotate=True, angle=0.0), P(rotate=True, angle=2.0),
        P(shift=(sr, sc, 0)), P(shift=(sr, sc, 1)), P(shift=(0, 0, 1)), P(noise=True),
        P(flip=True, shift=(sr, 1, 1), clip=box), P(flip=True, reduc=True, contrast=True, clip=box, shift=(2, sc, 0), noise=True),
        P(flip=True, reduc=True, contrast=True, clip=box, rotate=True, angle=1.4, shift=(sr, sc, 1), noise=True),
        P(reduc=True, contrast=True, rotate=True, angle=0.6, noise=True),
    ]


_CACHE = {}


def _case(shape_name):
    """(records, noise field, parameter sets, restatement outputs fp64 / longdouble-or-None), computed once per shape."""
    if shape_name not in _CACHE:
        N, H, W, Cc = SHAPES[shape_name]
        rng = np.random.default_rng(len(shape_name))
        sets = _param_sets(H, W)
        if shape_name == "full":                                           # one batch: every step on and off, angles 0 and 2.0 included
            sets = [sets[14], sets[6], sets[13], sets[7]]
        recs = [R.record(rng, H, W, Cc) for _ in sets]
        recs[0][:, :, -1] -= recs[0][:, :, -1]                             # exact zeros next to -0.0: the two zeros in the select
        recs[0][0, 0, -1] = -0.0
        field = rng.standard_normal((len(sets), H, W, Cc - 1))
        ref = [R.dataAug(x, p, f) for x, p, f in zip(recs, sets, field)]
        ld = [R.dataAug(x, p, f, np.longdouble) if p["rotate"] else None for x, p, f in zip(recs, sets, field)]
        for r in ref:
            r.setflags(write=False)
        _CACHE[shape_name] = (np.stack(recs), field, sets, ref, ld)
    return _CACHE[shape_name]


def _run(x, sets, field, lo, hi):
    from ultrasound_modeling_amd.DataFilePlayGround import dataAug_batch
    xin = torch.from_numpy(x[lo:hi]).to(DEV)
    keep = xin.clone()
    out = dataAug_batch(xin, sets[lo:hi], noise=torch.from_numpy(field[lo:hi]).to(DEV))
    assert torch.equal(_bits(xin), _bits(keep)), "the input was modified"
    assert out.data_ptr() != xin.data_ptr() and out.shape == xin.shape and out.dtype == torch.float64
    return out.cpu().numpy()


def _compare(got, ref, ld, p, tag):
    if not p["rotate"]:
        assert np.array_equal(got, ref), (tag, np.abs(got - ref).max())
        return 0.0, 0.0
    worst = (0.0, 0.0)
    for c in range(ref.shape[2]):
        own = float(np.abs(ref[:, :, c] - ld[:, :, c]).max())
        bound = max(8 * own, 2.0 ** -50 * float(np.abs(ref[:, :, c]).max()))
        err = float(np.abs(got[:, :, c] - ld[:, :, c]).max())
        print(f"{tag} plane {c}: device error {err:.3e}, restatement's own {own:.3e}, bound {bound:.3e}")
        assert err <= bound, (tag, c, err, bound)
        worst = max(worst, (err, bound))
    assert ((got == 0) == (ref == 0)).all(), tag                           # the zero frame outside the rotated image is the same
    return worst


@pytest.mark.parametrize("shape_name", sorted(SHAPES))
def test_steps_and_chain_match_restatement(shape_name):
    N = SHAPES[shape_name][0]
    x, field, sets, ref, ld = _case(shape_name)
    worst = (0.0, 0.0)
    for lo in range(0, len(sets), N):
        hi = min(lo + N, len(sets))
        got = _run(x, sets, field, lo, hi)
        for k in range(lo, hi):
            worst = max(worst, _compare(got[k - lo], ref[k], ld[k], sets[k], f"{shape_name}[{k}]"))
    print(f"{shape_name}: largest rotation error {worst[0]:.3e} (its bound {worst[1]:.3e})")
    # the restatement's branches were all taken: contrast changed something, the gate and the clip box zeroed something
    k = 3
    assert not np.array_equal(ref[k] if shape_name != "full" else ref[0], x[k] if shape_name != "full" else x[0])


def test_contrast_skip_rule_on_the_device():
    from ultrasound_modeling_amd.DataFilePlayGround import dataAug_batch
    const = np.full((8, 8, 4), 3.0)
    const[:, :, 0] = 1.0                                                   # hi == lo
    same = np.full((10, 10, 3), 1.0)
    same[0, 0, 1] = 0.0                                                    # hi != lo, but both percentiles are 1.0
    for img in (const, same):
        assert np.array_equal(R.contrast(img), img)
        out = dataAug_batch(torch.from_numpy(img[None]).to(DEV), [R.params(contrast=True)])
        assert np.array_equal(out[0].cpu().numpy(), img)


@pytest.mark.parametrize("shape_name", ["small", "odd"])
def test_masking_is_per_sample(shape_name):
    x, field, sets, _, _ = _case(shape_name)
    order = [14, 0, 3, 7, 12, 11, 15, 4]                                   # rotating and non-rotating samples interleaved
    xb, fb, sb = x[order], field[order], [sets[k] for k in order]
    batch = _run(xb, sb, fb, 0, len(order))
    for k in range(len(order)):
        one = _run(xb, sb, fb, k, k + 1)
        assert np.array_equal(batch[k].view(np.int64), one[0].view(np.int64)), (shape_name, k)


def test_determinism_and_generated_noise():
    from ultrasound_modeling_amd.DataFilePlayGround import dataAug, dataAug_batch, draw_aug
    x, _, sets, _, _ = _case("small")
    order = [14, 11, 0, 15, 13]
    xin = torch.from_numpy(x[order]).to(DEV)
    ps = [dict(sets[k], seed=1000 + k) for k in order]
    used = torch.full((len(order),) + x.shape[1:3] + (x.shape[3] - 1,), 7.0, dtype=torch.float64, device=DEV)
    a = dataAug_batch(xin, ps, noise_out=used)
    b = dataAug_batch(xin, ps)
    assert torch.equal(_bits(a), _bits(b))
    c = dataAug_batch(xin, ps, noise=used)
    assert torch.equal(_bits(a), _bits(c))
    u = used.cpu().numpy()
    assert (u[2] == 0).all() and abs(u[0].std() - 1) < 0.05 and abs(u[0].mean()) < 0.05 and not np.array_equal(u[0], u[1])
    one = dataAug_batch(xin[3:4], ps[3:4])                                 # the generated field does not depend on the batch position
    assert torch.equal(_bits(one[0]), _bits(a[3]))
    rng1, rng2 = random.Random(5), random.Random(5)
    drawn = dataAug_batch(xin, rng=rng1)
    assert torch.equal(_bits(drawn), _bits(dataAug_batch(xin, [draw_aug(rng2) for _ in order])))
    random.seed(11)
    single = dataAug(xin[0])
    random.seed(11)
    assert single.shape == xin[0].shape and torch.equal(_bits(single), _bits(dataAug_batch(xin[:1], [draw_aug()])[0]))


def test_dataaug_batch_rejects_bad_input():
    from ultrasound_modeling_amd.DataFilePlayGround import dataAug_batch
    ok = torch.zeros((1, 8, 8, 3), dtype=torch.float64, device=DEV)
    for bad in (ok.float(), ok[0], ok.cpu(), ok[:, :3], ok[:, :, :3], ok[..., :2]):
        with pytest.raises(ValueError):
            dataAug_batch(bad, [R.params()] * bad.shape[0])
    with pytest.raises(ValueError):
        dataAug_batch(ok, [R.params(), R.params()])
    with pytest.raises(ValueError):
        dataAug_batch(ok, [R.params(noise=True)], noise=torch.zeros((1, 8, 8, 3), dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ oversampling end to end
def _tree(root):
    from scipy.io import savemat
    rng = np.random.default_rng(9)
    for p, cycles, bleed in ((2, 1, True), (3, 2, False), (8, 1, False), (9, 2, True), (12, 1, True)):
        d = os.path.join(root, "DoD%03d" % p)
        os.makedirs(d)
        m = PR.make_mat(rng, H0=37, W0=23, C=cycles, nan_blood=False)
        Hm, Wm = m["bloodMask"].shape
        m["bloodMask"] = np.zeros((Hm, Wm))
        m["normalMask"] = np.ones((Hm, Wm))
        if bleed:
            m["bloodMask"][Hm // 3:Hm // 3 + 3, Wm // 4:Wm // 4 + 2] = 2.0
        savemat(os.path.join(d, "DoD%03d_Ter001_RC1_Displacement_Polar.mat" % p), m)
    return root


def test_oversampling_end_to_end(tmp_path):
    from ultrasound_modeling_amd.DataFilePlayGround import build_arrays, dataAug_batch, draw_aug, patient_plan, permutation, REDUC_ONLY
    raw = _tree(str(tmp_path / "raw"))
    plan = patient_plan(1, raw)
    train0, test0, trp0, tep0 = build_arrays(1, 1, raw, seed=7)
    train, test, trp, tep = build_arrays(1, 1, raw, seed=7, oversample="bleed")
    assert np.array_equal(test, test0) and np.array_equal(tep, tep0)
    again = build_arrays(1, 1, raw, seed=7, oversample="bleed")
    assert np.array_equal(train, again[0]) and np.array_equal(trp, again[2])
    inv, inv0 = np.argsort(permutation(len(trp), 7)), np.argsort(permutation(len(trp0), 7))
    data, names, data0, names0 = train[inv], trp[inv, 0], train0[inv0], trp0[inv0, 0]
    rng = random.Random(7)
    row, row0, seen = 0, 0, set()
    for name, _, is_test in plan:
        if is_test:
            continue
        patient = int(name[-3:])
        base = name + "_Ter001_RC1"
        while row0 < len(names0) and names0[row0] == base:
            orig = data0[row0]
            assert names[row] == base and np.array_equal(data[row].view(np.int64), orig.view(np.int64))    # byte-equal originals
            f = R.bleed_fraction(orig[0])
            expect = R.plan(base, patient, f, "bleed")
            assert len(expect) == (2 if patient in R.IPH else 0) + (int(f / 0.03) if f > 0.05 else 0)
            row, row0 = row + 1, row0 + 1
            for row_name, kind in expect:
                assert names[row] == row_name
                p = dict(REDUC_ONLY) if kind == "reduc" else draw_aug(rng)
                ref = dataAug_batch(torch.from_numpy(orig).to(DEV), [p])[0].cpu().numpy()
                assert np.array_equal(data[row, 0].view(np.int64), ref.view(np.int64)), row_name
                if kind == "reduc":
                    assert np.array_equal(ref, R.reduc(orig[0]))
                seen.add(kind + ("+rot" if p["rotate"] else ""))
                row += 1
    assert row == len(names) and row0 == len(names0) and len(names) > len(names0)
    assert {"reduc", "aug+rot"} <= seen, seen
