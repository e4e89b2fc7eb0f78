"""tests/fused_restatement.py (the fp64 stage functions test_gpu_fused_routes.py holds the fused tile kernels to) against
oracle/usseg_oracle.py, on the CPU: composing the forward stages without rounding is the oracle's conv2d_same / layer_norm / leaky_relu /
batch_norm / avg_pool2 chain, the backward stages are torch.autograd.grad through that chain (fp64, ~1e-12 relative, a tiny shape per
configuration), the restated launcher arithmetic gives the grids the GPU cases rely on, and the seeds and shapes of the GPU file's
cardinal_bwd cases keep the kink-excluded share of every dx check within KINK_FRAC - with the fp64 chain rounded to bf16 at the storage
points as the stand-in for the tensor the kernel stores (dv)."""
import pytest
import torch
import torch.nn.functional as F

import fused_restatement as FR
import usseg_oracle as O
from route_probe import KINK_FRAC, bf

TOL = 1e-12
SMALL = [(1, 8, 8), (3, 2, 6), (3, 16, 5), (2, 24, 40), (2, 13, 19)]


def close(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), (what, err)


def groups_ln(x, gamma, beta, G):
    cg = x.shape[-1] // G
    return torch.cat([O.layer_norm(x[..., g * cg:(g + 1) * cg], gamma[g * cg:(g + 1) * cg], beta[g * cg:(g + 1) * cg], eps=1e-3) for g in range(G)], -1)


@pytest.mark.parametrize("cfg", FR.CONFIGS, ids=[f"c{c[0]}" for c in FR.CONFIGS])
def test_cardinal_stages_are_the_oracle_chain_and_its_gradient(cfg):
    cin, cv11, cvkk, oc = cfg
    U, V, Up, Vp = FR.dims(cfg)
    B, H, W = 2, 5, 6
    p = FR.card_weights(cfg)
    k = p["keras"]
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(B, H, W, cin, generator=gen, dtype=torch.float64)
    got = FR.card_chain(x, p, cfg, rounded=False)
    u_raw = O.conv2d_same(x, k["w1"], p["b1"]).requires_grad_(True)
    u = O.leaky_relu(groups_ln(u_raw, p["g1"], p["be1"], 3))
    v_raw = O.conv2d_same(u, k["w2"], p["b2"])
    v_raw.retain_grad()
    y = O.leaky_relu(groups_ln(v_raw, p["g2"], p["be2"], 3))
    sc_raw = O.conv2d_same(x, k["wsc"], p["bsc"]).requires_grad_(True)
    sc = O.leaky_relu(O.layer_norm(sc_raw, p["gsc"], p["besc"], eps=1e-3))
    for nm, t in (("u_raw", u_raw), ("u", u), ("v_raw", v_raw), ("y", y), ("sc_raw", sc_raw), ("sc", sc)):
        close(got[nm], t.detach(), nm)
    rows, _ = FR.tile_sums(got["y"])
    close(rows.sum(1) / (H * W), O.avg_pool2(F.pad(got["y"], (0, 0, 0, 0, 0, 1)))[:, :0].sum((1, 2)) + got["y"].mean((1, 2)), "gap rows")
    # backward: dL/dy = mult*s[b]*dout + dg[b] (the split-attention re-weighting's backward), dL/dsc = dsc
    dout, dsc = torch.randn(B, H, W, V, generator=gen, dtype=torch.float64), torch.randn(B, H, W, oc, generator=gen, dtype=torch.float64)
    s, dg = torch.rand(B, V, generator=gen, dtype=torch.float64), 0.05 * torch.randn(B, V, generator=gen, dtype=torch.float64)
    g1, g2 = p["g1"].clone().requires_grad_(True), p["g2"].clone().requires_grad_(True)
    u2 = O.leaky_relu(groups_ln(u_raw, g1, p["be1"], 3))
    v2 = O.conv2d_same(u2, k["w2"], p["b2"])
    v2.retain_grad()
    y2 = O.leaky_relu(groups_ln(v2, g2, p["be2"], 3))
    (y2 * (3.0 * s[:, None, None, :] * dout + dg[:, None, None, :])).sum().backward()
    r2 = FR.fuse_bwd(v_raw.detach(), dout, p["g2"], p["be2"], s, dg, 3.0)
    close(r2["dx"].reshape(B, H, W, V), v2.grad, "dv")
    close(r2["dgamma"], g2.grad, "dgamma2")
    r1 = FR.conv1_bwd(u_raw.detach(), F.pad(v2.grad, (0, Vp - V)), p["w2d"], p["g1"], p["be1"])
    close(r1["dx"].reshape(B, H, W, U), u_raw.grad, "dcat[:U]")
    close(r1["dgamma"], g1.grad, "dgamma1")
    (gs,) = torch.autograd.grad((sc * dsc).sum(), sc_raw)
    close(FR.ln_lrelu(sc_raw.detach(), p["gsc"], p["besc"], 1, dy=dsc)["dx"].reshape(B, H, W, oc), gs, "dcat[Up:]")


def test_stem_stages_are_the_oracle_chain_and_its_gradient():
    B, H, W = 2, 6, 8
    gen = torch.Generator().manual_seed(32)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    w1, w2, w3 = rn(3, 3, 1, 16) / 3, rn(3, 3, 16, 32) / 12, rn(3, 3, 32, 32) / 17
    b1, b2, b3, gamma, beta, mean, var = rn(16), rn(32), rn(32), 1 + 0.2 * rn(32), rn(32), rn(32), 0.5 + torch.rand(32, generator=gen, dtype=torch.float64)
    x = rn(B, H, W, 1)
    y1 = FR.lrelu(FR.conv_fwd(F.pad(x, (0, 7)), FR.pack_f(w1, 8, 16), b1, 9, 16)[0])
    t1 = FR.lrelu(FR.conv_fwd(y1, FR.pack_f(w2, 16, 32), b2, 9, 32)[0])
    c2 = FR.conv_fwd(t1, FR.pack_f(w3, 32, 32), b3, 9, 32)[0]
    pooled = FR.bn_lrelu_pool(c2, gamma, beta, mean, var, O.KERAS["bn_eps"])[0]
    oy1 = O.leaky_relu(O.conv2d_same(x, w1, b1))
    ot1 = O.leaky_relu(O.conv2d_same(oy1, w2, b2))
    oc2 = O.conv2d_same(ot1, w3, b3)
    op = O.avg_pool2(O.leaky_relu(O.batch_norm(oc2, gamma, beta, mean, var, training=False)))
    for nm, a, b in (("y1", y1, oy1), ("t1", t1, ot1), ("c2", c2, oc2), ("pooled", pooled, op)):
        close(a, b, nm)
    # conv3_dgrad_actbwd: mode 0 in front of convtmp_1 (16 channels), mode 2 in front of convtmp_2 (32 channels, folded BatchNorm)
    dy = rn(B, H, W, 32)
    pre = rn(B, H, W, 16).requires_grad_(True)
    (O.conv2d_same(O.leaky_relu(pre), w2) * dy).sum().backward()
    close(FR.dgrad_actbwd(dy, FR.pack_d(w2, 32, 16), O.leaky_relu(pre).detach(), 0)["dx"], pre.grad, "mode 0 dx")
    xin, g, b = rn(B, H, W, 32).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    g.data[::3] *= -1
    act = O.leaky_relu(O.batch_norm(xin, g, b, mean, var, training=False))
    (O.conv2d_same(act, w3) * dy).sum().backward()
    r = FR.dgrad_actbwd(dy, FR.pack_d(w3, 32, 32), act.detach(), 2, g.detach(), b.detach(), var, O.KERAS["bn_eps"])
    close(r["dx"], xin.grad, "mode 2 dx")
    close(r["dgamma"], g.grad, "mode 2 dgamma")
    close(r["dbeta"], b.grad, "mode 2 dbeta")
    close(r["dbias"], xin.grad.sum((0, 1, 2)), "mode 2 dbias")


def test_launcher_arithmetic():
    lds = [FR.card_bwd_lds(c) for c in FR.CONFIGS]
    assert lds[0] == 54272 and lds[3] == 156672, lds
    for c in FR.CONFIGS:
        for shape in SMALL:
            nt, sct, G = FR.card_bwd_grid(c, *shape)
            assert G == max(nt, sct) <= 256 and FR.walk(nt, G) == "one"
        assert FR.card_bwd_grid(c, 5, 56, 60) == (280, 263, 256) and FR.card_bwd_grid(c, 3, 100, 76)[::2] == (390, 256)
        assert FR.card_bwd_grid(c, 2, 160, 160)[::2] == (800, 256)
    assert FR.walk(280, 256) == "second" and FR.walk(800, 256) == "three+" and FR.walk(1125, 512) == "three+" and FR.walk(546, 512) == "second"
    assert FR.card_bwd_grid(FR.CONFIGS[3], 2, 160, 160, g_env=613)[2] == 306 and FR.card_bwd_grid(FR.CONFIGS[3], 2, 160, 160, g_env=612)[2] == 612


@pytest.mark.parametrize("cfg,shape", [(c, s) for c in FR.CONFIGS for s in SMALL] + [(FR.CONFIGS[0], (5, 56, 60))],
                         ids=lambda v: "x".join(map(str, v)))
def test_kink_share_of_the_gpu_cases(cfg, shape):
    """The three dx checks of a cardinal_bwd case leave out at most KINK_FRAC of their elements."""
    p, i = FR.card_weights(cfg), FR.card_bwd_inputs(cfg, *shape)
    U, V, Up, Vp = FR.dims(cfg)
    r2 = FR.fuse_bwd(i["v_raw"], i["dout"], p["g2"], p["be2"], i["sa_s"], i["sa_dg"], 3.0)
    dv = F.pad(bf(r2["dx"]).reshape(*shape, V), (0, Vp - V))
    r1 = FR.conv1_bwd(i["u_raw"], dv, p["w2d"], p["g1"], p["be1"])
    rs = FR.ln_lrelu(i["sc_raw"], p["gsc"], p["besc"], 1, dy=i["dsc"])
    for nm, r in (("dv", r2), ("dcat[:U]", r1), ("dcat[Up:]", rs)):
        assert FR.kink_share(r) <= KINK_FRAC, (nm, FR.kink_share(r))
