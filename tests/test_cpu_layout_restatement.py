"""The restatements of tests/layout_restatement.py against independent statements of the same operations (CPU, fp64 where arithmetic is
involved): pack_ref against kernel.permute(...) for the operand orders the layers emit, quad_unpack_ref / quad_bias_fold_ref against
autograd through the oracle's transposed convolution, ops.make_pack_tilemap against tilemap_ref / tile_cover, and the two BatchNorm
constant restatements against the oracle's BatchNormalization."""
import math

import pytest
import torch
import torch.nn.functional as F

import layout_restatement as LR
import usseg_oracle as O

BF = torch.bfloat16
up = lambda v, m: (v + m - 1) // m * m


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ packs
@pytest.mark.parametrize("k,cin,cout", [(3, 5, 7), (1, 20, 12), (3, 40, 72)])
def test_pack_ref_conv2d_orders(k, cin, cout):
    """The two jobs of layers.Conv2D.pack_jobs: forward rows = out channel, K = tap*cin_p + ci; dgrad rows = in channel, K = tap*cout_p + co."""
    T, cin_p, cout_p = k * k, up(cin, 8), up(cout, 8)
    w = torch.randn(k, k, cin, cout, generator=gen(1))
    sT, sI, sO = cin * cout, cout, 1
    f, fm = LR.pack_ref(w, sT, sO, sI, T, cout, cin, (up(cout_p, 16), T * cin_p), T * cin_p, cin_p, 0, 0)
    want = w.permute(3, 0, 1, 2).reshape(cout, T, cin).to(BF)
    assert torch.equal(f.reshape(-1, T, cin_p)[:cout, :, :cin], want)
    assert fm.reshape(-1, T, cin_p)[:cout, :, :cin].all() and int(fm.sum()) == T * cin * cout
    assert f[~fm].abs().max().item() == 0 if (~fm).any() else True
    d, dm = LR.pack_ref(w, sT, sI, sO, T, cin, cout, (up(cin_p, 16), T * cout_p), T * cout_p, cout_p, 0, 0)
    assert torch.equal(d.reshape(-1, T, cout_p)[:cin, :, :cout], w.reshape(T, cin, cout).permute(1, 0, 2).to(BF))
    assert int(dm.sum()) == T * cin * cout and dm.reshape(-1, T, cout_p)[:cin, :, :cout].all()


def test_pack_ref_grouped_slab_orders():
    """The four jobs per branch of the grouped slab (TBI_ResNest.py pack_jobs): block-diagonal placement by n_off / k_off, the 1x1 jobs with sT = 0."""
    G, cin, cv11, cvkk, T = 4, 20, 16, 24, 9
    cin_p, Up, Vp = up(cin, 8), G * cv11, G * cvkk
    k1 = [torch.randn(1, 1, cin, cv11, generator=gen(10 + g)) for g in range(G)]
    k2 = [torch.randn(3, 3, cv11, cvkk, generator=gen(20 + g)) for g in range(G)]
    shapes = dict(w1_f=(up(Up, 16), cin_p), w1_d=(up(cin_p, 16), Up), w2_f=(up(Vp, 16), T * Up), w2_d=(up(Up, 16), T * Vp))
    img = {n: torch.zeros(s, dtype=BF) for n, s in shapes.items()}
    cnt = {n: torch.zeros(s, dtype=torch.int64) for n, s in shapes.items()}
    sT = cv11 * cvkk
    for g in range(G):
        for name, args in (("w1_f", (k1[g], 0, 1, cv11, 1, cv11, cin, shapes["w1_f"], cin_p, cin_p, g * cv11, 0)),
                           ("w1_d", (k1[g], 0, cv11, 1, 1, cin, cv11, shapes["w1_d"], Up, Up, 0, g * cv11)),
                           ("w2_f", (k2[g], sT, 1, cvkk, T, cvkk, cv11, shapes["w2_f"], T * Up, Up, g * cvkk, g * cv11)),
                           ("w2_d", (k2[g], sT, cvkk, 1, T, cv11, cvkk, shapes["w2_d"], T * Vp, Vp, g * cv11, g * cvkk))):
            v, m = LR.pack_ref(*args)
            img[name][m] = v[m]
            cnt[name] += m
    for n in cnt:
        assert cnt[n].max().item() == 1, f"{n}: two branch jobs write one element"
    for g in range(G):
        assert torch.equal(img["w1_f"][g * cv11:(g + 1) * cv11, :cin], k1[g].reshape(cin, cv11).T.to(BF))
        assert torch.equal(img["w1_d"][:cin, g * cv11:(g + 1) * cv11], k1[g].reshape(cin, cv11).to(BF))
        f = img["w2_f"].reshape(-1, T, Up)[g * cvkk:(g + 1) * cvkk, :, g * cv11:(g + 1) * cv11]
        assert torch.equal(f, k2[g].reshape(T, cv11, cvkk).permute(2, 0, 1).to(BF))
        d = img["w2_d"].reshape(-1, T, Vp)[g * cv11:(g + 1) * cv11, :, g * cvkk:(g + 1) * cvkk]
        assert torch.equal(d, k2[g].reshape(T, cv11, cvkk).permute(1, 0, 2).to(BF))
    # everything off the diagonal blocks was left alone
    assert int(cnt["w2_f"].sum()) == G * T * cv11 * cvkk and int(cnt["w1_f"].sum()) == G * cin * cv11


def test_pack_ref_nscale_and_rounding():
    """One fp32 multiply, one round-to-nearest-even: 1 + 2^-8 is a bf16 tie (-> 1.0), 1 + 2^-7 + 2^-8 ties up to 1 + 2^-6; nscale follows n."""
    src = torch.tensor([[1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23], [3.0, 5.0, 7.0]])
    ns = torch.tensor([1.0, -0.5, 9.0])
    img, mask = LR.pack_ref(src, 0, 3, 1, 1, 2, 3, (4, 8), 8, 8, 1, 2, nscale=ns)
    assert img[1, 2:5].tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert img[2, 2:5].tolist() == [-1.5, -2.5, -3.5]
    assert int(mask.sum()) == 6 and mask[1:3, 2:5].all()
    fp = LR.job_footprint((0, 0, 0, 3, 1, 1, 2, 3, 8, 8, 1, 2, 0, 0))
    assert fp.tolist() == mask.reshape(-1).nonzero().reshape(-1).tolist()


# ------------------------------------------------------------------------------------------------ quad form against autograd
def _d2s(y4, Np, Cout):
    """[B,H,W,4*Np] -> [B,2H,2W,Cout]: full[b, 2i+a, 2j+b', n] = quad[b, i, j, (2a+b')*Np + n]."""
    B, H, W, _ = y4.shape
    return y4.reshape(B, H, W, 2, 2, Np)[..., :Cout].permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, Cout)


@pytest.mark.parametrize("k", [3, 4])
def test_quad_unpack_ref_against_autograd(k):
    B, H, W, Cin, Cin_phys, Cout, Np = 2, 5, 4, 6, 8, 3, 4
    g = gen(30 + k)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, b, dy = r(B, H, W, Cin), r(k, k, Cout, Cin), r(Cout), r(B, 2 * H, 2 * W, Cout)
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = O.conv2d_transpose_s2_same(x, wl, bl)
    (want * dy).sum().backward()
    # the quad form: a 3x3 'same' convolution of the (channel-padded) input with the quad weight, then depth-to-space
    xq = F.pad(x, (0, Cin_phys - Cin))
    wq = LR.quad_weight(w, Np, Cin_phys).requires_grad_(True)              # [9][Cin_phys][4*Np] == Keras [3,3,Cin_phys,4*Np]
    bq = LR.quad_bias_expand_ref(b, Cout, Np).requires_grad_(True)
    y4 = O.conv2d_same(xq, wq.reshape(3, 3, Cin_phys, 4 * Np), bq)
    got = _d2s(y4, Np, Cout)
    assert (got - want.detach()).abs().max().item() < 1e-12
    (got * dy).sum().backward()
    grad0, db0 = r(k, k, Cout, Cin), r(Cout)
    fold = LR.quad_unpack_ref(wq.grad, Cin_phys, Cin, Cout, Np, k, grad0)
    assert (fold - (grad0 + wl.grad)).abs().max().item() < 1e-12
    dbias, mag = LR.quad_bias_fold_ref(bq.grad, Cout, Np, db0)
    assert (dbias - (db0 + dy.sum((0, 1, 2)))).abs().max().item() < 1e-12
    assert (dbias - (db0 + bl.grad)).abs().max().item() < 1e-12 and (mag >= dbias.abs() - 1e-12).all()


def test_quad_taps_agree_with_the_layers():
    """The (tap, class) the layers' pack_jobs compute with integer arithmetic are the ones derived from the parity identity."""
    for k in (3, 4):
        pad = 1 if k == 4 else 0
        for (kh, kw), (t, cls) in LR.quad_taps(k).items():
            a, b = (kh + pad) & 1, (kw + pad) & 1
            assert (t, cls) == (((a + pad - kh) // 2 + 1) * 3 + ((b + pad - kw) // 2 + 1), a * 2 + b)
        assert len({v for v in LR.quad_taps(k).values()}) == k * k


def test_quad_bias_expand_ref():
    b = torch.tensor([1.0, 2.0, 3.0])
    assert LR.quad_bias_expand_ref(b, 3, 4).tolist() == [1, 2, 3, 0] * 4
    assert LR.quad_bias_expand_ref(torch.arange(1.0, 6.0), 5, 8).reshape(4, 8)[2].tolist() == [1, 2, 3, 4, 5, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ tilemap
def _fake_job(T, Nn, Kk):
    return (0, 0, 0, 0, 0, T, Nn, Kk, Kk, Kk, 0, 0, 0, 0)


TILE_JOBS = [_fake_job(1, 5, 7), _fake_job(3, 32, 32), _fake_job(1, 64, 64), _fake_job(5, 1, 1), _fake_job(577, 1, 1)]


@pytest.mark.parametrize("tpb", [1, 4])
def test_make_pack_tilemap_against_tilemap_ref(tpb):
    from ultrasound_modeling_amd import ops
    assert [LR.job_tiles(j) for j in TILE_JOBS] == [1, 3, 4, 5, 577]
    for jobs in (TILE_JOBS, TILE_JOBS[::-1], TILE_JOBS[4:], TILE_JOBS[:1]):
        tm, nblocks = ops.make_pack_tilemap(jobs, "cpu", tpb)
        assert tm.dtype == torch.int32 and tm.numel() == 3 * nblocks
        ref = LR.tilemap_ref(jobs, tpb)
        assert torch.equal(tm.reshape(-1, 3).long(), ref)
        assert nblocks == sum(math.ceil(LR.job_tiles(j) / tpb) for j in jobs)
        assert (tm.reshape(-1, 3)[:, 2] >= 1).all(), "a triple of no tile"
        for c in LR.tile_cover(jobs, tm):
            assert (c == 1).all()


def test_tile_cover_sees_a_dropped_and_a_doubled_tile():
    tm = LR.tilemap_ref(TILE_JOBS, 4)
    short = tm.clone()
    short[-1, 2] -= 1
    if short[-1, 2] == 0:
        short = short[:-1]
    assert (LR.tile_cover(TILE_JOBS, short)[-1] == 0).sum().item() == 1
    twice = torch.cat([tm, tm[:1]])
    assert LR.tile_cover(TILE_JOBS, twice)[0].max().item() == 2
    with pytest.raises(AssertionError):
        LR.tile_cover(TILE_JOBS, torch.tensor([[0, 0, 2]]))


# ------------------------------------------------------------------------------------------------ BatchNorm constants
@pytest.mark.parametrize("with_bias", [True, False])
def test_bn_fold_ref_against_the_oracle(with_bias):
    C, Cp = 21, 24
    g = gen(40)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    gamma, beta, mean, var, bias, conv = r(C), r(C), r(C), r(C).abs() + 0.1, r(C), r(7, C)
    eps = O.KERAS["bn_eps"]
    sc, sh, scm, shm = LR.bn_fold_ref(gamma, beta, mean, var, bias if with_bias else None, C, Cp, eps)
    want = O.batch_norm(conv + (bias if with_bias else 0), gamma, beta, mean, var, training=False)
    # eps enters as the fp32 value the kernel argument holds: 1e-3 differs from it by 5e-11, relative to var + eps >= 0.1
    assert ((sc[:C] * conv + sh[:C]) - want).abs().max().item() < 1e-8
    e64 = float(torch.tensor(eps, dtype=torch.float32))
    exact = (conv + (bias if with_bias else 0) - mean) / torch.sqrt(var + e64) * gamma + beta
    assert ((sc[:C] * conv + sh[:C]) - exact).abs().max().item() < 1e-12
    assert sc[C:].abs().max().item() == 0 and sh[C:].abs().max().item() == 0 and sc.numel() == sh.numel() == Cp
    assert (scm >= sc.abs()).all() and (shm >= sh.abs() - 1e-15).all()


def test_bn_finalize_ref_against_the_oracle():
    g = gen(41)
    x = torch.randn(64, 9, generator=g, dtype=torch.float64) * torch.linspace(0.5, 3, 9, dtype=torch.float64) + torch.linspace(-2, 2, 9, dtype=torch.float64)
    mm0, mv0 = torch.randn(9, generator=g, dtype=torch.float64), torch.rand(9, generator=g, dtype=torch.float64) + 0.5
    mom = 0.5                                   # exact in fp32, so the comparison below holds to rounding
    r = LR.bn_finalize_ref(x.sum(0), (x * x).sum(0), 64, mom, mm0, mv0)
    assert (r["mean"] - x.mean(0)).abs().max().item() < 1e-12
    assert (r["var"] - x.var(0, unbiased=False)).abs().max().item() < 1e-12
    assert (r["var_mag"] >= r["var"]).all() and (r["mean_mag"] >= r["mean"].abs() - 1e-15).all()
    assert (r["mm"] - (mm0 * mom + x.mean(0) * (1 - mom))).abs().max().item() < 1e-12
    assert (r["mv"] - (mv0 * mom + x.var(0, unbiased=False) * (1 - mom))).abs().max().item() < 1e-12
    # Keras' training-mode layer (momentum 0.99, an fp32 argument: compare at the fp32 value)
    m32 = float(torch.tensor(O.KERAS["bn_momentum"], dtype=torch.float32))
    _, (mm, mv) = O.batch_norm(x, torch.ones(9, dtype=torch.float64), torch.zeros(9, dtype=torch.float64), mm0, mv0, training=True)
    r = LR.bn_finalize_ref(x.sum(0), (x * x).sum(0), 64, O.KERAS["bn_momentum"], mm0, mv0)
    dm = abs(m32 - O.KERAS["bn_momentum"])      # what the fp32 argument differs from 0.99 by, times the two terms it multiplies
    assert ((r["mm"] - mm).abs() <= dm * (mm0.abs() + x.mean(0).abs()) + 1e-12).all()
    assert ((r["mv"] - mv).abs() <= dm * (mv0.abs() + x.var(0, unbiased=False)) + 1e-12).all()
    # the stored statistics, when given, are what the moving update reads
    r2 = LR.bn_finalize_ref(x.sum(0), (x * x).sum(0), 64, 0.5, mm0, mv0, stored=(torch.zeros(9), torch.ones(9)))
    assert torch.equal(r2["mm"], mm0 * 0.5) and torch.equal(r2["mv"], mv0 * 0.5 + 0.5)
    # a cancelling channel never goes negative
    s, s2 = torch.tensor([100.0]), torch.tensor([100.0 * 100.0 - 1e-9])
    assert LR.bn_finalize_ref(s, s2, 1, 0.5)["var"].item() == 0.0


# ------------------------------------------------------------------------------------------------ unpack
def test_unpack_ref_inverts_pack_ref():
    """Scattering a [T][Mrows][Ncols] scratch back through unpack_ref with the strides of the forward pack returns the packed block."""
    T, cin, cout, Mrows, Ncols = 9, 5, 7, 8, 8
    w = torch.randn(T, cin, cout, generator=gen(50))                       # Keras [tap][in][out]
    scratch = torch.zeros(T, Mrows, Ncols)
    scratch[:, :cin, :cout] = w                                            # m = input channel, n = output channel
    d0 = torch.randn(T * cin * cout + 5, generator=gen(51))
    ref, mag, mask = LR.unpack_ref(scratch, Mrows, Ncols, T, cout, cin, 0, 0, d0, cin * cout, 1, cout, 0.5, True)
    assert torch.equal(ref[:-5].reshape(T, cin, cout), d0[:-5].double().reshape(T, cin, cout) + 0.5 * w.double())
    assert torch.equal(ref[-5:], d0[-5:].double()) and mask[:-5].all() and not mask[-5:].any()
    assert torch.equal(mag[:-5].reshape(T, cin, cout), d0[:-5].double().abs().reshape(T, cin, cout) + 0.5 * w.double().abs())
    ref, mag, mask = LR.unpack_ref(scratch, Mrows, Ncols, T, cout, cin, 0, 0, d0, cin * cout, cin, 1, -2.0, False)   # [tap][out][in]
    assert torch.equal(ref[:-5].reshape(T, cout, cin), -2.0 * w.double().permute(0, 2, 1))
    # a block of the scratch at (k_off, n_off)
    ref, _, mask = LR.unpack_ref(scratch, Mrows, Ncols, 1, 2, 3, 4, 1, torch.zeros(6), 0, 3, 1, 1.0, True)
    assert torch.equal(ref.reshape(2, 3), w[0, 1:4, 4:6].double().T)
