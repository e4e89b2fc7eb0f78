"""tests/pointwise_restatement.py on the CPU: every restatement against torch autograd of an independently written forward (backward
forms) or against the oracle function it restates (forward forms), in fp64 to 1e-12; and, on the very inputs and shapes the GPU route matrix
(tests/test_gpu_pointwise_routes.py) uses, the conditions it relies on: bf16-exact activation inputs (no element is ever left out of an
activation check), loss cases whose clip-edge set is at most 0.1 % of the pixels and whose forced row is clipped on every class in fp64, and
every grid property the GPU cases assert."""
import pytest
import torch
import torch.nn.functional as F

import loss_restatement as R
import pointwise_restatement as PR
import usseg_oracle as O
from route_probe import ACTS

TOL = 1e-12


def close(a, b, what=""):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert ((a - b).abs() <= TOL * (1.0 + b.abs())).all(), (what, (a - b).abs().max().item())


@pytest.fixture(scope="module")
def gen():
    return torch.Generator().manual_seed(1357)


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("act", list(ACTS))
def test_activation_forms(gen, act):
    x = torch.randn(3, 5, 7, 8, generator=gen, dtype=torch.float64)
    dy = torch.randn(3, 5, 7, 8, generator=gen, dtype=torch.float64)
    slope = ACTS[act][1]
    # (F.leaky_relu rounds its slope to float32 even on a float64 tensor, so LeakyReLU is written with two clamps)
    indep = {"none": lambda v: v, "lrelu": lambda v: v.clamp(min=0) + slope * v.clamp(max=0), "relu": F.relu, "elu": lambda v: F.elu(v, slope)}[act]
    y, ymag = PR.act_fwd_ref(x, act)
    close(y, indep(x), act)
    close(ymag, indep(x).abs())
    if act == "lrelu":
        slope = float(torch.tensor(slope, dtype=torch.float32))          # route_probe.act_d's slope is the float32 0.3 the kernels are handed
    xr = x.clone().requires_grad_(True)
    (indep(xr) * dy).sum().backward()
    dx, dxmag = PR.act_bwd_ref(x, dy, act)
    close(dx, xr.grad, act)
    close(dxmag, xr.grad.abs())


def test_pool_forms(gen):
    x = torch.randn(2, 6, 10, 5, generator=gen, dtype=torch.float64)
    y, ymag = PR.pool_fwd_ref(x)
    close(y, O.avg_pool2(x))
    close(ymag, O.avg_pool2(x.abs()))
    dy, add = torch.randn(2, 3, 5, 5, generator=gen, dtype=torch.float64), torch.randn(2, 6, 10, 5, generator=gen, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    (F.avg_pool2d(xr.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * dy).sum().backward()
    close(PR.pool_bwd_ref(dy)[0], xr.grad)
    close(PR.pool_bwd_ref(dy)[1], xr.grad.abs())
    close(PR.pool_bwd_ref(dy, add)[0], xr.grad + add)
    close(PR.pool_bwd_ref(dy, add)[1], xr.grad.abs() + add.abs())


def test_column_sums_and_reinject(gen):
    x = torch.randn(37, 11, generator=gen, dtype=torch.float64)
    close(PR.colsum_ref(x)[0], torch.ones(37, dtype=torch.float64) @ x)
    close(PR.colsum_ref(x)[1], torch.ones(37, dtype=torch.float64) @ x.abs())
    close(PR.colsumsq_ref(x)[0], torch.einsum("mc,mc->c", x, x))
    for _id, hshape, views in PR.REINJECT_CASES[:3]:
        h = torch.randn(hshape, generator=gen, dtype=torch.float64).requires_grad_(True)
        shapes = [v[0] for v in views]
        outs = PR.reinject_fwd_ref(h, shapes)
        for o, s in zip(outs, shapes):                                   # Decoder.py:140-141: tf.reshape of the row-major hidden state
            close(o.detach().reshape(-1), h.detach().reshape(-1))
            assert tuple(o.shape) == s
        gs = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
        sum((o * g).sum() for o, g in zip(outs, gs)).backward()
        d, mag = PR.reinject_bwd_ref(gs, hshape)
        close(d, h.grad)
        close(mag, sum(g.abs().reshape(hshape) for g in gs))
    full = torch.randn(2, 6, 10, 8, generator=gen, dtype=torch.float64)
    q = PR.s2d_ref(full, 16)
    for (b, i, j, a, c, n) in [(0, 0, 0, 0, 0, 0), (1, 2, 4, 1, 1, 7), (1, 1, 3, 1, 0, 5), (0, 2, 0, 0, 1, 2)]:
        assert q[b, i, j, (2 * a + c) * 16 + n] == full[b, 2 * i + a, 2 * j + c, n]
    assert torch.isnan(q[..., 8:16]).all() and int(torch.isnan(q).sum()) == q.numel() // 2


@pytest.mark.parametrize("C", [3, 2, 4, 8])
def test_loss_forms(C):
    B, H, W = 2, 9, 11
    logits, y = PR.loss_inputs(0, C, B, H, W)
    inv = PR.loss_inv(B)
    r = PR.cce_from_logits(logits, y, inv)
    close(r["probs"], O.softmax_lastaxis(logits))
    close(r["loss"], O.compute_loss(y, O.softmax_lastaxis(logits), B + 2))
    close(r["lossmag"], r["loss"])                                       # every term of the clipped cross-entropy is >= 0
    # dlogits: autograd of an independently written forward (probabilities, division by the class sum, clamp)
    z = logits.clone().requires_grad_(True)
    p = torch.exp(z - z.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    q = (p / p.sum(-1, keepdim=True)).clamp(1e-7, 1.0 - 1e-7)
    (-((y * 0.9 + 0.1 / C) * q.log()).sum() * inv).backward()
    close(r["dlogits"], z.grad)
    close(r["dlogits"], r["probs"] * (r["dLdp"] - (r["dLdp"] * r["probs"]).sum(-1, keepdim=True)))      # the chain rule the mag is built on
    close(r["mag"], r["probs"] * (r["dLdp"].abs() + (r["dLdp"].abs() * r["probs"]).sum(-1, keepdim=True)))
    assert all(r["dLdp"][px].abs().max().item() == 0 for px in PR.forced_rows(B, H, W))
    # my_loss_cat
    m = PR.cat_from_logits(logits, y)
    close(m["scale"], 1.0 / (y.sum(0) + 1.0) / (H * W))
    if C == 3:
        close(m["loss"], O.my_loss_cat(y, m["probs"], H, W))
        close(PR.loss_cat_map(y, m["probs"], m["scale"])[0], O.my_loss_cat(y, m["probs"], H, W))
    z = logits.clone().requires_grad_(True)
    p = torch.softmax(z, -1)
    tot = sum(-(y[..., c] * torch.log(p[..., c] + 1e-7)).sum(0) / (y[..., c].sum(0) + 1.0) / (H * W) for c in range(C)).sum()
    tot.backward()
    close(m["dlogits"], z.grad)
    close(m["loss"].sum(), tot.detach())
    assert not m["edge"].any()
    # the class loss goes through tests/loss_restatement.py (checked by tests/test_cpu_class_loss.py)
    k = PR.class_from_logits(logits, y, *R.form(PR.LOSS_FORM, C), inv)
    close(k["loss"], R.scalar(y, k["probs"], *R.form(PR.LOSS_FORM, C), 1.0 / inv))
    close(k["lossmag"], k["loss"])


def test_adam_form(gen):
    n = 1000
    p, g, m, v = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(4))
    v = v.abs() * 1e-3
    b1, b2, eps = O.KERAS["adam_beta1"], O.KERAS["adam_beta2"], O.KERAS["adam_eps"]
    for clip in (1.0, 1e9, 0.0):
        sumsq = float((g * g).sum())
        for step in (1, 3):
            r = PR.adam_ref(p, g, m, v, sumsq, clip, PR.lr_t_ref(step, 1e-3, b1, b2), b1=b1, b2=b2, eps=eps)
            gc = O.clip_by_global_norm([g], clip)[0] if clip > 0 else [g]
            po, mo, vo = [p.clone()], [m.clone()], [v.clone()]
            O.adam_step(po, gc, mo, vo, step, 1e-3)
            close(r["p"], po[0])
            close(r["m"], mo[0])
            close(r["v"], vo[0])
    # decoupled decay (tfa DecoupledWeightDecayExtension: p -= wd_t*p before the Adam update), masked
    mask = PR.decay_mask(n)
    r = PR.adam_ref(p, g, m, v, sumsq, 1.0, 2e-3, wd_t=3e-2, mask=mask, b1=b1, b2=b2, eps=eps)
    u = PR.adam_ref(torch.where(mask.bool(), p - 3e-2 * p, p), g, m, v, sumsq, 1.0, 2e-3, b1=b1, b2=b2, eps=eps)
    close(r["p"], u["p"])
    close(r["pmag"], p.abs() + (3e-2 * p * mask).abs() + (2e-3 * r["m"] / (r["v"].sqrt() + eps)).abs())
    close(r["mmag"], b1 * m.abs() + (1 - b1) * (g * r["scale"]).abs())
    close(r["vmag"], b2 * v + (1 - b2) * (g * r["scale"]) ** 2)


# ------------------------------------------------------------------------------------------------ what the GPU cases rely on
def test_activation_inputs_are_bf16_exact():
    for i, (_id, (B, H, W), C, _view) in enumerate(PR.ACT_CASES):
        for seed in (100 + i, 200 + i):
            x = PR.seam_bf16(seed, B, H, W, C)
            assert x.dtype == torch.bfloat16
            x64 = x.double()
            assert torch.equal(x64.to(torch.bfloat16).double(), x64) and torch.isfinite(x64).all()
            assert x64[-1, -1, -1, -1] == 64 and x64[0, H // 2, 0, 0] == -48


@pytest.mark.parametrize("case", PR.LOSS_CASES, ids=[c[0] for c in PR.LOSS_CASES])
def test_loss_cases_edges_forced_row_and_grids(case):
    _id, kind, C, B, H, W, quad = case
    HW = H * W
    logits, y = PR.loss_inputs(kind, C, B, H, W)
    r = PR.loss_ref(kind, C, logits, y, PR.loss_inv(B))
    if kind != 1:
        # the forced row is clipped on every class in fp64 by orders of magnitude, so in any arithmetic: exactly no gradient.  It is checked, not
        # left out (its saturated class lies within 2^-20 of the upper clip constant in ABSOLUTE terms, which is what the edge rule measures)
        lo, hi = (PR.CCE_EPS, 1.0 - PR.CCE_EPS) if kind == 0 else (R.LO, R.HI)
        for px in PR.forced_rows(B, H, W):
            assert r["dLdp"][px].abs().max().item() == 0
            assert r["probs"][px].max().item() > hi and r["probs"][px].sort().values[-2].item() < 1e-3 * lo
            r["edge"][px] = False
    n_edge = int(r["edge"].sum())
    assert n_edge <= 1e-3 * B * HW, (n_edge, B * HW)
    assert torch.isfinite(r["dlogits"]).all() and torch.isfinite(r["loss"]).all()
    PR.loss_grid_properties(case)


def test_walk_grids():
    PR.walk_properties()


def test_colsum_grids():
    assert [PR.colsum_plan(1, C)["lpp"] for C in PR.COLSUM_C_ONE] == [1, 1, 4, 16, 64, 64]
    assert PR.colsum_plan(1, 1000)["last_slab"] == 488 and PR.colsum_plan(1, 1000)["nslab"] == 2
    assert PR.colsum_plan(10 ** 9, 3072)["cap"] == 3072 // 6 == 512 == PR.colsum_plan(10 ** 9, 3072)["grid"]
    assert PR.colsum_plan(10 ** 9, 16384)["cap"] == 96 and PR.colsum_plan(10 ** 9, 520)["cap"] == 1024
    for C, kind in PR.COLSUM_CASES:
        _M, pl = PR.colsum_properties(C, kind)
        assert (pl["nslab"] > 1) == (C > 512)
        if C <= 512:
            PR.colsum_properties(C, kind, slabs=False)                              # channel_stats
    for C, kind, _add in PR.POOL_COLSUM_CASES:
        B, H, W = PR.pool_colsum_shape(C, kind)
        PR.colsum_properties(C, kind, rows=4, slabs=False, M=B * H * W)


def test_optimiser_and_probability_loss_grids():
    PR.optimiser_properties()
    for n in PR.ADAM_N:
        k = PR.decay_mask(n)
        assert k[n - 3:].all() and (n < 4 or not k[0])
        p, g, m, v, still = PR.optim_inputs(n)
        assert still.any() and (g[still] == 0).all() and (m[still] == 0).all() and (v[still] == 0).all()
        assert n < 8 or torch.signbit(p[still]).any()
    PR.probs_properties()


def test_cast_ties_are_ties():
    x = PR.cast_ties((2, 5, 7, 3), torch.float64)
    f32 = x.float()
    tie = (f32.view(torch.int32) & 0xFFFF) == 0x8000                   # the fp32 value lies exactly between two bf16 values ...
    assert int(tie.sum()) >= 16
    off, two_step = (x - f32.double())[tie], f32.to(torch.bfloat16).double()[tie] - f32.double()[tie]
    assert (off != 0).all() and (off * two_step < 0).all()             # ... the fp64 value on the side AWAY from where ties-to-even sends it
    assert torch.equal(PR.cast_ties((2, 5, 7, 3), torch.float32).double().float(), PR.cast_ties((2, 5, 7, 3), torch.float32))
