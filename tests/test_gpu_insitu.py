"""Per-layer IN-SITU parity (GPU): north_star's "per-layer fwd/bwd within 1e-3 rel of reference on identical inputs".

The whole Arch B network (ResNest.py encoder + patch embedding + Decoder.py, 64x64x1, B=2) is run ONCE in the oracle with
bf16 storage emulation and a recorder around its primitives; the recorded tensors of every layer - its input and the gradient
that arrives at its output - are bf16-representable, so they can be handed to the product EXACTLY.  Then every kernel launch of
the product's forward and backward pass is replayed one layer at a time, through the model's own modules and packed operands
(grouped split-attention GEMMs, multi-job dilated branches, fused four-branch backward-data, quad-form head ...), on the
oracle's input for that layer, and compared with that layer recomputed locally in fp64 (with the fusion the product uses, so
there is exactly one bf16 rounding on either side):

    bf16 outputs (activations, input gradients)  <= 1e-3 relative L2 against the fp64 result rounded to bf16
    fp32 outputs (weight / bias / norm-parameter gradients, probabilities, loss)  <= 1e-3 against fp64

Conv kernels are bf16-representable here (the product's MFMA operands ARE the bf16 rounding of its fp32 masters, so this
removes the operand rounding from both sides); every other parameter is arbitrary fp32.
"""
import pytest
import torch

import usseg_oracle as O
from route_probe import routed, small_deferral

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
ENC = "transformer.embeddings.hybrid_model."


def bf(t):
    return t.detach().to(torch.bfloat16).to(torch.float64)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def dev(t64, cp=None):
    """fp64 NHWC (bf16-representable) -> device bf16 with zero pad channels."""
    B, H, W, C = t64.shape
    cp = cp or (C + 7) // 8 * 8
    out = torch.zeros(B, H, W, cp, dtype=torch.bfloat16)
    out[..., :C] = t64.detach().to(torch.bfloat16)
    return out.to(DEV)


class Recorder:
    """Wraps the oracle's primitives; keeps (input, output) of every call, keyed by the parameter the call used."""
    NAMES = ("conv2d_same", "conv2d_transpose_s2_same", "layer_norm", "batch_norm", "leaky_relu", "avg_pool2", "split_attention")

    def __init__(self, P):
        self.id2name = {id(v): k for k, v in P.items()}
        self.conv, self.norm, self.sa, self.pool, self.acts = {}, {}, {}, [], []
        self.orig = {n: getattr(O, n) for n in self.NAMES}
        self.in_sa = 0

    def _keep(self, t):
        if t.requires_grad:
            t.retain_grad()
        return t

    def __enter__(self):
        o, rec = self.orig, self

        def conv2d_same(x, w, b=None, dilation=1):
            y = o["conv2d_same"](x, w, b, dilation)
            if not rec.in_sa:
                rec.conv[rec.id2name[id(w)][:-len(".kernel")]] = (x, rec._keep(y), dilation)
            return y

        def conv2d_transpose_s2_same(x, w, b=None):
            y = o["conv2d_transpose_s2_same"](x, w, b)
            rec.conv[rec.id2name[id(w)][:-len(".kernel")]] = (x, rec._keep(y), 1)
            return y

        def layer_norm(x, gamma, beta, eps=None):
            y = o["layer_norm"](x, gamma, beta, eps)
            if not rec.in_sa:
                rec.norm[rec.id2name[id(gamma)][:-len(".gamma")]] = (x, y)
            return y

        def batch_norm(x, gamma, beta, mm, mv, training=None):
            y = o["batch_norm"](x, gamma, beta, mm, mv, training)
            rec.norm[rec.id2name[id(gamma)][:-len(".gamma")]] = (x, y)
            return y

        def leaky_relu(x):
            y = o["leaky_relu"](x)
            if not rec.in_sa:
                rec.acts.append((x, rec._keep(y)))           # (input kept alive, output)
            return y

        def avg_pool2(x):
            y = o["avg_pool2"](x)
            rec.pool.append((x, rec._keep(y)))
            return y

        def split_attention(inputs, P, prefix, radix, norm="ln"):
            rec.in_sa += 1
            try:
                y = o["split_attention"](inputs, P, prefix, radix, norm)
            finally:
                rec.in_sa -= 1
            rec.sa[prefix] = (inputs[0], rec._keep(y))
            return y
        for n, f in (("conv2d_same", conv2d_same), ("conv2d_transpose_s2_same", conv2d_transpose_s2_same), ("layer_norm", layer_norm),
                     ("batch_norm", batch_norm), ("leaky_relu", leaky_relu), ("avg_pool2", avg_pool2), ("split_attention", split_attention)):
            setattr(O, n, f)
        return self

    def __exit__(self, *a):
        for n, f in self.orig.items():
            setattr(O, n, f)

    def act_after(self, x):
        """The recorded LeakyReLU output whose input was the tensor ``x`` (same object, or an equal concatenation)."""
        for xi, yi in self.acts:
            if xi is x:
                return yi
        for xi, yi in self.acts:
            if xi.shape == x.shape and torch.equal(xi.detach(), x.detach()):
                return yi
        raise KeyError("no activation recorded for this tensor")


@pytest.fixture(scope="module")
def world():
    """(product model, parameters, recorder) after one recorded oracle forward+backward with bf16 storage emulation."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    P = O.init_vision_transformer_params(channel=1, seed=13, perturb=True)
    P = {k: (bf(v) if k.endswith(".kernel") else v.float().double()) for k, v in P.items()}
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1)
    net.load_params(P)
    x, y = O.synthetic_batch(2, 64, 64, 1, seed=14)
    names = O.trainable_names(P)
    leaves = {n: P[n].clone().requires_grad_(True) for n in names}
    Pl = dict(P)
    Pl.update(leaves)
    rec = Recorder(Pl)
    O.STORAGE_DTYPE = torch.bfloat16
    try:
        with rec:
            probs = O.vision_transformer_forward(bf(x), Pl, 3, 3, as_executed=False)
            O.compute_loss(y, probs, 2).backward()
    finally:
        O.STORAGE_DTYPE = None
    rec.P, rec.x, rec.y = P, bf(x), y
    return net, P, rec


def g_of(t):
    """The gradient that arrived at a recorded tensor, as the product would hold it (bf16)."""
    assert t.grad is not None
    return bf(t.grad)


def fresh(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def check(name, got, want, tol=TOL, worst=None):
    e = rel(got, want)
    if worst is not None:
        worst.append((e, name))
    assert e < tol, f"{name}: rel {e:.3e} >= {tol:g}"
    return e


# ------------------------------------------------------------------------------------------------ plain conv layers
def conv_layer_check(net, rec, P, name, layer, worst, act=False, residual=None, transposed=False):
    """One Conv2D / Conv2DTranspose of the model on the oracle's input: forward (+ fused LeakyReLU / residual), backward-data,
    weight and bias gradients."""
    from ultrasound_modeling_amd import ops
    x, y, dil = rec.conv[name]
    x, dy = x.detach(), g_of(y)
    xl, wl, bl = fresh(x, P[name + ".kernel"], P[name + ".bias"])
    f = O.conv2d_transpose_s2_same if transposed else (lambda a, w, b: O.conv2d_same(a, w, b, dil))
    ref = f(xl, wl, bl)
    out_ref = O.leaky_relu(ref) if act else ref
    if residual is not None:
        out_ref = out_ref + residual
    xd = dev(x, layer.cin_p)
    kw = dict(act=ops.ACT_LRELU, alpha=0.3) if act else {}
    if residual is not None:
        kw["residual"] = dev(residual)
    out = layer.forward(xd, **kw)
    check(name + " fwd", out[..., :layer.cout], bf(out_ref), worst=worst)
    if layer.cout_p > layer.cout:
        assert out[..., layer.cout:].abs().max().item() == 0, name + ": pad channels"
    gx, gw, gb = torch.autograd.grad(ref, [xl, wl, bl], dy)
    net.flat.zero_grad()
    dx = layer.backward(dev(dy, layer.cout_p))
    torch.cuda.synchronize()
    check(name + " dgrad", dx[..., :layer.cin], bf(gx), worst=worst)
    check(name + " wgrad", layer.kernel.grad, gw, worst=worst)
    check(name + " dbias", layer.bias.grad, gb, worst=worst)


def norm_layer_check(net, rec, P, name, layer, worst, kind):
    """LayerNormalization / inference BatchNormalization + fused LeakyReLU: forward, dx, dgamma, dbeta and the producing conv's
    bias gradient (sum of dx)."""
    from ultrasound_modeling_amd import ops
    x, y = rec.norm[name]
    dy = g_of(rec.act_after(y))
    xl, gl, bl = fresh(x, P[name + ".gamma"], P[name + ".beta"])
    if kind == "ln":
        ref = O.leaky_relu(O.layer_norm(xl, gl, bl))
    else:
        ref = O.leaky_relu(O.batch_norm(xl, gl, bl, P[name + ".moving_mean"], P[name + ".moving_variance"]))
    out = layer.forward(dev(x), ops.ACT_LRELU, 0.3)
    C = x.shape[-1]
    check(name + " fwd", out[..., :C], bf(ref), worst=worst)
    gx, gg, gb = torch.autograd.grad(ref, [xl, gl, bl], dy)
    net.flat.zero_grad()
    dbias = torch.zeros((C + 7) // 8 * 8, dtype=torch.float32, device=DEV)
    dx = layer.backward(dev(dy), dbias=dbias)
    torch.cuda.synchronize()
    check(name + " dx", dx[..., :C], bf(gx), worst=worst)
    check(name + " dgamma", layer.gamma.grad, gg, worst=worst)
    check(name + " dbeta", layer.beta.grad, gb, worst=worst)
    check(name + " dbias(sum dx)", dbias[:C], gx.sum(dim=(0, 1, 2)), worst=worst)


def folded_reference(x, P, cname, bname, dil):
    """conv + inference BatchNorm + LeakyReLU with the operand the folded launch documents: W' = bf16(W * s), s = gamma * rsqrt(var +
    eps) in fp32, shift = beta - mean*s + s*bias in fp32 - then fp64 arithmetic.  (With bf16-representable W the UNFOLDED launch has
    an exact operand; the folded one rounds W*s, exactly as any launch rounds arbitrary fp32 master weights: ~2-3e-3 on the output,
    which the second bar below records.)"""
    g32, b32 = P[bname + ".gamma"].float(), P[bname + ".beta"].float()
    s32 = g32 * torch.rsqrt(P[bname + ".moving_variance"].float() + 1e-3)
    shift = (b32 - P[bname + ".moving_mean"].float() * s32 + s32 * P[cname + ".bias"].float()).double()
    w = bf(P[cname + ".kernel"].float() * s32)
    return O.leaky_relu(O.conv2d_same(x, w, None, dil) + shift)


def folded_conv_bn_check(net, rec, P, cname, bname, conv, bn, worst):
    """conv -> inference BatchNorm -> LeakyReLU as ONE launch (the BN scale folded into the packed forward operand, its shift as
    the bias): forward against the fp64 composite, then the backward the model runs - norm backward from the ACTIVATED output
    (mode 2), conv backward-data and weight gradient with the UNFOLDED operands."""
    from ultrasound_modeling_amd import ops
    x, y_conv, dil = rec.conv[cname]
    x = x.detach()
    y_bn = rec.norm[bname][1]
    act_rec = rec.act_after(y_bn)
    dy = g_of(act_rec)
    xl, wl, bl, gl, btl = fresh(x, P[cname + ".kernel"], P[cname + ".bias"], P[bname + ".gamma"], P[bname + ".beta"])
    ref = O.leaky_relu(O.batch_norm(O.conv2d_same(xl, wl, bl, dil), gl, btl, P[bname + ".moving_mean"], P[bname + ".moving_variance"]))
    out = conv.forward(dev(x, conv.cin_p), act=ops.ACT_LRELU, alpha=0.3, bias=bn.fold_shift)
    check(cname + "+bn+act fwd (folded)", out[..., :conv.cout], bf(folded_reference(x, P, cname, bname, dil)), worst=worst)
    check(cname + "+bn+act fwd (folded) vs the unfolded fp64 composite", out[..., :conv.cout], bf(ref), 5 * TOL, worst=worst)
    # ---- backward, step 1: BatchNorm + LeakyReLU backward FROM THE ACTIVATED TENSOR the forward stored (mode 2).  The slope mask
    # is the sign of that stored tensor, so the fp64 expectation is evaluated on the product's own output `out` (a reference
    # that re-derived the signs from an unfolded forward would disagree wherever |pre-activation| is below the operand rounding).
    yq = out[..., :conv.cout].double().cpu()
    gam, bet = P[bname + ".gamma"], P[bname + ".beta"]
    rstd = torch.rsqrt(P[bname + ".moving_variance"] + 1e-3)
    slope = torch.where(yq > 0, torch.ones_like(yq), torch.full_like(yq, 0.3))
    pre = torch.where(yq >= 0, yq, yq / 0.3)
    xh = (pre - bet) / gam
    dh = dy * slope
    net.flat.zero_grad()
    d_raw = bn.backward_folded(out, dev(dy), ops.ACT_LRELU, 0.3, dbias=conv.bias.grad)
    torch.cuda.synchronize()
    check(bname + " dx (mode 2)", d_raw[..., :conv.cout], bf(dh * gam * rstd), worst=worst)
    check(bname + " dgamma (mode 2)", bn.gamma.grad, (dh * xh).sum(dim=(0, 1, 2)), worst=worst)
    check(bname + " dbeta (mode 2)", bn.beta.grad, dh.sum(dim=(0, 1, 2)), worst=worst)
    check(cname + " dbias (mode 2)", conv.bias.grad, (dh * gam * rstd).sum(dim=(0, 1, 2)), worst=worst)
    # ---- step 2: the conv's backward-data and weight gradient on that d_raw, with the UNFOLDED operands
    dr = d_raw[..., :conv.cout].double().cpu()
    gx, gw = torch.autograd.grad(O.conv2d_same(xl, wl, None, dil), [xl, wl], dr)
    net.flat.zero_grad()
    dx = conv.backward(d_raw, skip_bias=True)
    torch.cuda.synchronize()
    check(cname + " dgrad", dx[..., :conv.cin], bf(gx), worst=worst)
    check(cname + " wgrad", conv.kernel.grad, gw, worst=worst)


def test_stem_and_pools(world):
    from ultrasound_modeling_amd import ops
    net, P, rec = world
    enc = net.transformer.embeddings.hybrid_model
    worst = []
    # conv1 (+ fused LeakyReLU, ResNest.py:39-40): no input gradient
    name = ENC + "conv1"
    x, y, _ = rec.conv[name]
    xl, wl, bl = fresh(x, P[name + ".kernel"], P[name + ".bias"])
    ref = O.conv2d_same(xl, wl, bl)
    out = enc.conv1.forward(dev(x.detach(), 8), act=ops.ACT_LRELU, alpha=0.3)
    check(name + " fwd", out[..., :16], bf(O.leaky_relu(ref)), worst=worst)
    dy = g_of(y)
    _, gw, gb = torch.autograd.grad(ref, [xl, wl, bl], dy)
    net.flat.zero_grad()
    enc.conv1.backward(dev(dy), need_dx=False)
    torch.cuda.synchronize()
    check(name + " wgrad", enc.conv1.kernel.grad, gw, worst=worst)
    check(name + " dbias", enc.conv1.bias.grad, gb, worst=worst)
    if enc.convtmp_1.fold_scale() is None:
        conv_layer_check(net, rec, P, ENC + "convtmp_1", enc.convtmp_1, worst)
        norm_layer_check(net, rec, P, ENC + "convtmp_1bn", enc.convtmp_1bn, worst, "bn")
    else:
        folded_conv_bn_check(net, rec, P, ENC + "convtmp_1", ENC + "convtmp_1bn", enc.convtmp_1, enc.convtmp_1bn, worst)
    conv_layer_check(net, rec, P, ENC + "convtmp_2", enc.convtmp_2, worst)
    norm_layer_check(net, rec, P, ENC + "convtmp_2bn", enc.convtmp_2bn, worst, "bn")
    for i, pool in enumerate((enc.conv1_pool, enc.conv2_pool, enc.conv3_pool, enc.conv4_pool)):
        x, y = rec.pool[i]
        xl, = fresh(x)
        ref = O.avg_pool2(xl)
        out = pool.forward(dev(x))
        check(f"pool{i} fwd", out, bf(ref), worst=worst)
        dy = g_of(y)
        dx = pool.backward(dev(dy))
        check(f"pool{i} bwd", dx, bf(torch.autograd.grad(ref, xl, dy)[0]), worst=worst)
    # ---- the fused stem launch (csrc/stem.hip): conv1 + act -> convtmp_1 + folded BN + act -> convtmp_2 -> BN + act + pool from ONE read of x.
    # Its only input is x, so the inner tensors are compared with the oracle's own chain (same bf16 storage points).
    if enc.convtmp_1.fold_scale() is not None:
        fw = []
        x0 = rec.conv[ENC + "conv1"][0].detach()
        bn1, bn2 = enc.convtmp_1bn, enc.convtmp_2bn
        y1f, t1f, c2f, pf = ops.stem_fwd(dev(x0, 8), enc.conv1.wp_f, enc.conv1.bias.data, enc.convtmp_1.wp_f, bn1.fold_shift, enc.convtmp_2.wp_f,
                                         enc.convtmp_2.bias.data, bn2.gamma.data, bn2.beta.data, bn2.moving_mean_p, bn2.moving_variance_p, bn2.eps, 0.3)
        torch.cuda.synchronize()
        check("fused stem: conv1 + act", y1f, rec.act_after(rec.conv[ENC + "conv1"][1]), worst=fw)
        # convtmp_1 runs with the BatchNorm scale folded into its bf16 operand (one more operand rounding than the oracle's unfolded chain:
        # the 5e-3 bar of the folded launch above), and convtmp_2 / the pool inherit its output
        check("fused stem: convtmp_1 + bn + act", t1f, rec.act_after(rec.norm[ENC + "convtmp_1bn"][1]), 5 * TOL, worst=fw)
        check("fused stem: convtmp_2 (pre-norm)", c2f, rec.conv[ENC + "convtmp_2"][1], 5 * TOL, worst=fw)
        check("fused stem: bn + act + pool", pf, rec.pool[0][1], 5 * TOL, worst=fw)
        # against the product's own four launches on the same input: the same arithmetic at the same rounding points
        y1u = enc.conv1.forward(dev(x0, 8), act=ops.ACT_LRELU, alpha=0.3)
        t1u = enc.convtmp_1.forward(y1u, act=ops.ACT_LRELU, alpha=0.3, bias=bn1.fold_shift)
        c2u = enc.convtmp_2.forward(t1u)
        pu = bn2.forward_pool(c2u, ops.ACT_LRELU, 0.3)
        for nm, f_, u_ in (("y1", y1f, y1u), ("t1", t1f, t1u), ("c2", c2f, c2u), ("pooled", pf, pu)):
            check(f"fused stem vs the four launches: {nm}", f_, u_, worst=fw)
        print("fused stem:", [(f"{e:.2e}", n) for e, n in sorted(fw, reverse=True)[:8]])
    print("stem/pools worst:", sorted(worst, reverse=True)[:4])


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_residual_S_stage_layer_by_layer(world, stage):
    """conv_{stage}: the grouped 1x1 GEMM, per-group LayerNorm, block-diagonal 3x3, split attention, shortcut and concats_2,
    each on the oracle's own input for that layer."""
    from ultrasound_modeling_amd import ops
    net, P, rec = world
    st = getattr(net.transformer.embeddings.hybrid_model, f"conv_{stage}")
    grp = st._group
    pre = f"{ENC}conv_{stage}."
    cards = [f"{pre}cardinal_blocks.{k}." for k in range(3)]
    worst = []
    a = 0.3
    x = rec.conv[cards[0] + "conv1"][0].detach()                 # the stage input (shared by the three paths and the shortcut)
    xd = dev(x, grp.cin_p)
    B, H, W, _ = x.shape

    def cat_pad(ts, width):
        return dev(torch.cat([t.detach() for t in ts], dim=3), width)

    # ---- conv1 of the three paths as ONE GEMM (ResNest.py:139)
    leaf = {c: fresh(P[c + "conv1.kernel"], P[c + "conv1.bias"]) for c in cards}
    xl, = fresh(x)
    refs = [O.conv2d_same(xl, *leaf[c]) for c in cards]
    u_raw = ops.conv2d_fwd(xd, grp.w1_f, grp.b1, 1, 1, ops.new_act(B, H, W, grp.Up, DEV))
    check("grouped conv1 fwd", u_raw[..., :grp.U], bf(torch.cat(refs, 3)), worst=worst)
    assert grp.Up == grp.U or u_raw[..., grp.U:].abs().max().item() == 0
    dys = [g_of(rec.conv[c + "conv1"][1]) for c in cards]
    grads = torch.autograd.grad(refs, [xl] + [t for c in cards for t in leaf[c]], dys)
    du_raw = cat_pad(dys, grp.Up)
    dx = ops.conv2d_dgrad(du_raw, grp.w1_d, 1, 1, ops.new_act(B, H, W, grp.cin_p, DEV))
    check("grouped conv1 dgrad", dx[..., :grp.cin], bf(grads[0]), worst=worst)
    net.flat.zero_grad()
    ops.conv2d_wgrad_mapped(xd, du_raw, 1, 1, grp._maps()[0])
    torch.cuda.synchronize()
    for k, c in enumerate(st.cardinal_blocks):
        check(f"grouped conv1 wgrad path {k}", c.conv1.kernel.grad, grads[1 + 2 * k], worst=worst)

    # ---- per-group LayerNorm + LeakyReLU (ResNest.py:140-141), one launch for the three paths
    def group_norm(tag, width, gam, bet, dgam, dbet, dbias, conv_tag):
        xs = [rec.norm[c + tag][0].detach() for c in cards]
        ys = [rec.norm[c + tag][1] for c in cards]
        lv = [fresh(xq, P[c + tag + ".gamma"], P[c + tag + ".beta"]) for xq, c in zip(xs, cards)]
        refs_ = [O.leaky_relu(O.layer_norm(*l)) for l in lv]
        C = xs[0].shape[-1]
        xin = cat_pad(xs, width)
        out = ops.norm_act_fwd(xin, 3 * C, gam, bet, torch.empty_like(xin), 0, 3, 1e-3, ops.ACT_LRELU, a)
        check(f"{tag} fwd", out[..., :3 * C], bf(torch.cat(refs_, 3)), worst=worst)
        assert width == 3 * C or out[..., 3 * C:].abs().max().item() == 0
        dys_ = [g_of(rec.act_after(yq)) for yq in ys]
        gr = torch.autograd.grad(refs_, [t for l in lv for t in l], dys_)
        net.flat.zero_grad()
        dxn = ops.norm_act_bwd(xin, cat_pad(dys_, width), 3 * C, gam, bet, torch.empty_like(xin), dgam, dbet, 0, 3, 1e-3, ops.ACT_LRELU, a, dbias=dbias)
        torch.cuda.synchronize()
        check(f"{tag} dx", dxn[..., :3 * C], bf(torch.cat(gr[0::3], 3)), worst=worst)
        check(f"{tag} dgamma", dgam[:3 * C], torch.cat(gr[1::3]), worst=worst)
        check(f"{tag} dbeta", dbet[:3 * C], torch.cat(gr[2::3]), worst=worst)
        check(f"{tag} conv bias grad", dbias[:3 * C], torch.cat([g.sum(dim=(0, 1, 2)) for g in gr[0::3]]), worst=worst)
    group_norm("conv1_bn", grp.Up, grp.g1, grp.be1, grp.dg1, grp.dbe1, grp.db1, "conv1")

    # ---- the three 3x3 convs as ONE block-diagonal implicit GEMM (ResNest.py:142)
    us = [rec.conv[c + "conv2"][0].detach() for c in cards]
    leaf2 = {c: fresh(P[c + "conv2.kernel"], P[c + "conv2.bias"]) for c in cards}
    uls = fresh(*us)
    refs = [O.conv2d_same(ul, *leaf2[c]) for ul, c in zip(uls, cards)]
    ud = cat_pad(us, grp.Up)
    v_raw = ops.conv2d_fwd(ud, grp.w2_f, grp.b2, grp.k, grp.dil, ops.new_act(B, H, W, grp.Vp, DEV))
    check("grouped conv2 fwd", v_raw[..., :grp.V], bf(torch.cat(refs, 3)), worst=worst)
    assert grp.Vp == grp.V or v_raw[..., grp.V:].abs().max().item() == 0
    dys = [g_of(rec.conv[c + "conv2"][1]) for c in cards]
    grads = torch.autograd.grad(refs, uls + [t for c in cards for t in leaf2[c]], dys)
    dv = cat_pad(dys, grp.Vp)
    du = ops.conv2d_dgrad(dv, grp.w2_d, grp.k, grp.dil, torch.empty_like(ud))
    check("grouped conv2 dgrad", du[..., :grp.U], bf(torch.cat(grads[:3], 3)), worst=worst)
    net.flat.zero_grad()
    ops.conv2d_wgrad_mapped(ud, dv, grp.k, grp.dil, grp._maps()[1])
    torch.cuda.synchronize()
    for k, c in enumerate(st.cardinal_blocks):
        check(f"grouped conv2 wgrad path {k}", c.conv2.kernel.grad, grads[3 + 2 * k], worst=worst)
    group_norm("conv2_bn", grp.Vp, grp.g2, grp.be2, grp.dg2, grp.dbe2, grp.db2, "conv2")

    # ---- split attention (ResNest.py:171-199): GAP -> MLP -> channel softmax -> re-weighting, and its backward
    ys = [rec.sa[c + "split."][0].detach() for c in cards]
    mlp_names = ("dense1.kernel", "dense1.bias", "dense1_bn.gamma", "dense1_bn.beta", "dense2.kernel", "dense2.bias")
    yls = fresh(*ys)
    Pl = dict(P)
    mlp_leaves = []
    for c in cards:
        lv = fresh(*[P[c + "split." + n] for n in mlp_names])
        Pl.update({c + "split." + n: t for n, t in zip(mlp_names, lv)})
        mlp_leaves.append(lv)
    refs = [O.split_attention([yl] * 3, Pl, c + "split.", 3) for yl, c in zip(yls, cards)]
    yd = cat_pad(ys, grp.Vp)
    d = grp._sa_desc(B, H * W)
    params = grp.mlp_p[:4] + (None, None) + grp.mlp_p[4:]
    out, g, s, ws = ops.splitattn_fwd(d, yd, params, ops.new_act(B, H, W, grp.Vp, DEV))
    check("split attention fwd", out[..., :grp.V], bf(torch.cat(refs, 3)), worst=worst)
    douts = [g_of(rec.sa[c + "split."][1]) for c in cards]
    grads = torch.autograd.grad(refs, yls + [t for lv in mlp_leaves for t in lv], douts)
    net.flat.zero_grad()
    dyd = ops.splitattn_bwd(d, yd, cat_pad(douts, grp.Vp), params, grp.mlp_g, g, s, ws, torch.empty_like(yd))
    torch.cuda.synchronize()
    check("split attention dy", dyd[..., :grp.V], bf(torch.cat(grads[:3], 3)), 2 * TOL, worst=worst)   # dy = dout*s + broadcast(GAP path): two roundings meet
    for k, c in enumerate(st.cardinal_blocks):
        mods = (c.split.dense1.kernel, c.split.dense1.bias, c.split.dense1_bn.gamma, c.split.dense1_bn.beta, c.split.dense2.kernel, c.split.dense2.bias)
        for n, m, want in zip(mlp_names, mods, grads[3 + 6 * k: 9 + 6 * k]):
            check(f"split attention d{n} path {k}", m.grad.reshape(want.shape), want, 2 * TOL, worst=worst)

    # ---- shortcut (ResNest.py:99-101) and concats_2 with the shortcut added in its epilogue (:98,:102)
    conv_layer_check(net, rec, P, pre + "convtmp_sc", st.convtmp_sc, worst)
    norm_layer_check(net, rec, P, pre + "convtmp_scbn", st.convtmp_scbn, worst, "ln")
    sc = rec.act_after(rec.norm[pre + "convtmp_scbn"][1]).detach()
    conv_layer_check(net, rec, P, pre + "concats_2", st.concats_2, worst, residual=sc)
    # ---- ONE backward-data GEMM for the grouped 1x1 and the shortcut 1x1 (both read the stage input, ResNest.py:99,139): K = [Up | Oc]
    if getattr(st, "wcat_d", None) is not None:
        xl2, = fresh(x)
        lw = [fresh(P[c + "conv1.kernel"], P[c + "conv1.bias"]) for c in cards]
        wsc, bsc = fresh(P[pre + "convtmp_sc.kernel"], P[pre + "convtmp_sc.bias"])
        outs = [O.conv2d_same(xl2, w_, b_) for w_, b_ in lw] + [O.conv2d_same(xl2, wsc, bsc)]
        dys2 = [g_of(rec.conv[c + "conv1"][1]) for c in cards] + [g_of(rec.conv[pre + "convtmp_sc"][1])]
        gx_both, = torch.autograd.grad(outs, [xl2], dys2)
        dcat = ops.new_act(B, H, W, grp.Up + st.convtmp_sc.cout_p, DEV, zero=True)
        dcat[..., :grp.Up] = cat_pad(dys2[:3], grp.Up)
        dcat[..., grp.Up:] = dev(dys2[3])
        dxm = ops.conv2d_dgrad(dcat, st.wcat_d, 1, 1, ops.new_act(B, H, W, grp.cin_p, DEV))
        check("merged 1x1 backward-data (cardinal group + shortcut)", dxm[..., :grp.cin], bf(gx_both), worst=worst)
    # (per-element bounds and multi-tile walks of both fused launches below: test_gpu_fused_routes.py)
    # ---- the fused launch (csrc/cardinal.hip): grouped 1x1 -> LN -> LeakyReLU -> grouped 3x3 -> LN -> LeakyReLU (+ pooled rows) and the
    # shortcut 1x1 -> LN -> LeakyReLU from ONE read of the stage input.  Its only input is x, so the later tensors are compared with the
    # oracle's own chain (same bf16 storage points): a value that lands on the other side of a rounding boundary moves the tensors behind it.
    if grp.fused_ok(st.convtmp_sc):
        fw = []
        u_raw_f, u_f, v_raw_f, y_f, gap_f, sc_raw_f, sc_f = ops.cardinal_fwd(
            xd, grp.w1_f, grp.b1, grp.g1, grp.be1, grp.w2_f, grp.b2, grp.g2, grp.be2, st.convtmp_sc.wp_f, st.convtmp_sc.bias.data,
            st.convtmp_scbn.gamma.data, st.convtmp_scbn.beta.data, grp.P, grp.cv11, grp.cvkk, grp.Up, grp.Vp, st.convtmp_sc.cout, 1e-3, a)
        torch.cuda.synchronize()
        cat = lambda ts: torch.cat([t.detach() for t in ts], 3)
        check("fused: grouped conv1", u_raw_f[..., :grp.U], cat([rec.conv[c + "conv1"][1] for c in cards]), worst=fw)
        check("fused: conv1_bn + act", u_f[..., :grp.U], cat([rec.act_after(rec.norm[c + "conv1_bn"][1]) for c in cards]), 2 * TOL, worst=fw)
        check("fused: grouped conv2", v_raw_f[..., :grp.V], cat([rec.conv[c + "conv2"][1] for c in cards]), 2 * TOL, worst=fw)
        check("fused: conv2_bn + act", y_f[..., :grp.V], cat([rec.sa[c + "split."][0] for c in cards]), 2 * TOL, worst=fw)
        check("fused: shortcut conv", sc_raw_f, rec.conv[pre + "convtmp_sc"][1], worst=fw)
        check("fused: shortcut LN + act", sc_f, sc, 2 * TOL, worst=fw)
        for t, wlog in ((u_raw_f, grp.U), (u_f, grp.U), (v_raw_f, grp.V), (y_f, grp.V)):
            assert t.shape[3] == wlog or t[..., wlog:].abs().max().item() == 0, "fused: pad channels"
        check("fused: pooled partial rows", gap_f[0].sum(dim=1)[:, :grp.V] / (H * W), y_f[..., :grp.V].double().mean(dim=(1, 2)), worst=fw)
        # against the product's own unfused launches on the same input: the same arithmetic at the same rounding points
        u_raw_u = ops.conv2d_fwd(xd, grp.w1_f, grp.b1, 1, 1, ops.new_act(B, H, W, grp.Up, DEV))
        u_u = ops.norm_act_fwd(u_raw_u, grp.U, grp.g1, grp.be1, torch.empty_like(u_raw_u), 0, 3, 1e-3, ops.ACT_LRELU, a)
        v_raw_u = ops.conv2d_fwd(u_u, grp.w2_f, grp.b2, grp.k, grp.dil, ops.new_act(B, H, W, grp.Vp, DEV))
        y_u = ops.norm_act_fwd(v_raw_u, grp.V, grp.g2, grp.be2, torch.empty_like(v_raw_u), 0, 3, 1e-3, ops.ACT_LRELU, a)
        for nm, f_, u_ in (("u_raw", u_raw_f, u_raw_u), ("u", u_f, u_u), ("v_raw", v_raw_f, v_raw_u), ("y", y_f, y_u)):
            check(f"fused vs unfused launches: {nm}", f_, u_, worst=fw)
        print(f"stage {stage} fused:", [(f"{e:.2e}", n) for e, n in sorted(fw, reverse=True)[:6]])
    # ---- the fused BACKWARD launch (csrc/cardinal.hip, K3 backward): re-weighting + conv2_bn backward -> grouped 3x3 backward-data -> conv1_bn
    # backward, and the shortcut norm's backward, on the oracle's saved tensors and incoming gradients.  dv sits directly behind the oracle's
    # inputs; du_raw is behind two more bf16 storage points of the product's own chain (dv, du), so it gets the two-rounding bar, and every
    # output is also compared with the product's unfused launches on the same inputs.
    if grp.fused_ok(st.convtmp_sc) and getattr(st, "wcat_d", None) is not None:
        bw = []
        oc = st.convtmp_sc.cout
        v_raw_o = cat_pad([rec.conv[c + "conv2"][1] for c in cards], grp.Vp)
        u_raw_o = cat_pad([rec.conv[c + "conv1"][1] for c in cards], grp.Up)
        sc_raw_o = dev(rec.conv[pre + "convtmp_sc"][1])
        dout_d = cat_pad(douts, grp.Vp)
        dsc_d = dev(g_of(rec.act_after(rec.norm[pre + "convtmp_scbn"][1])))
        scn = st.convtmp_scbn

        def run(fused, defer_floats=0):
            net.flat.zero_grad()
            sa_s, sa_dg = ops.splitattn_bwd(d, yd, dout_d, params, grp.mlp_g, g, s, ws, None)
            dcat_ = ops.new_act(B, H, W, grp.Up + oc, DEV)
            if fused:
                dv_ = torch.empty_like(v_raw_o)
                grads_ = (grp.dg2, grp.dbe2, grp.db2, grp.dg1, grp.dbe1, grp.db1, scn.gamma.grad, scn.beta.grad, st.convtmp_sc.bias.grad)
                launch = lambda: ops.cardinal_bwd(dout_d, dsc_d, v_raw_o, u_raw_o, sc_raw_o, grp.w2_d, grp.g2, grp.be2, grp.g1, grp.be1, scn.gamma.data,
                                                  scn.beta.data, sa_s, sa_dg, 3.0, dv_, dcat_, grads_, grp.cin_p, grp.P, grp.cv11, grp.cvkk, grp.Up,
                                                  grp.Vp, oc, 1e-3, a)
                if defer_floats:
                    def deferred():
                        with small_deferral(defer_floats):
                            launch()
                    _, names = routed(deferred, "cardinal_bwd_kernel<", "reduce_finish_batched_kernel")
                    assert "reduce_finish_kernel" not in names, names   # all three regions deferred, none in the caller's workspace
                else:
                    launch()
            else:
                dv_ = ops.norm_act_bwd_sa(v_raw_o, dout_d, grp.V, grp.g2, grp.be2, torch.empty_like(v_raw_o), grp.dg2, grp.dbe2, 0, 3, 1e-3,
                                          ops.ACT_LRELU, a, sa_s, sa_dg, 3.0, dbias=grp.db2)
                du_ = ops.conv2d_dgrad(dv_, grp.w2_d, grp.k, grp.dil, torch.empty_like(u_raw_o))
                ops.norm_act_bwd(u_raw_o, du_, grp.U, grp.g1, grp.be1, dcat_[..., :grp.Up], grp.dg1, grp.dbe1, 0, 3, 1e-3, ops.ACT_LRELU, a, dbias=grp.db1)
                ops.norm_act_bwd(sc_raw_o, dsc_d, oc, scn.gamma.data, scn.beta.data, dcat_[..., grp.Up:], scn.gamma.grad, scn.beta.grad, 0, 1, 1e-3,
                                 ops.ACT_LRELU, a, dbias=st.convtmp_sc.bias.grad)
            torch.cuda.synchronize()
            vecs = [t.detach().clone() for t in (grp.dg2, grp.dbe2, grp.db2, grp.dg1, grp.dbe1, grp.db1, scn.gamma.grad, scn.beta.grad,
                                                 st.convtmp_sc.bias.grad)]
            return dv_, dcat_, vecs
        dv_f, dcat_f, vec_f = run(True)
        dv_u, dcat_u, vec_u = run(False)
        # the three partial-row regions of the launch are reserved together: behind a first producer (64 floats), a deferral region of
        # exactly their size holds the first two but not the third, so the reservation flushes once and then places all three (the
        # shortcut's region requested on its own would go to offset 0 after the flush, across the first).  G workgroup pairs: the larger of
        # the 8x8-tile and 64-pixel shortcut-tile counts while that is at most 256 (cardinal.hip launch_bwd).  Bit for bit the undeferred launch.
        G = max(-(-H // 8) * -(-W // 8) * B, -(-B * H * W // 64))
        assert G <= 256
        n2, n1, nsc = 3 * G * grp.Vp, 3 * G * grp.Up, 3 * G * oc
        assert nsc > 64
        dv_d, dcat_d, vec_d = run(True, -(-n2 // 64) * 64 + -(-n1 // 64) * 64 + nsc)
        for nm, f_, d_ in zip(("dv", "dcat", "dgamma2", "dbeta2", "dbias2", "dgamma1", "dbeta1", "dbias1", "dgamma_sc", "dbeta_sc", "dbias_sc"),
                              [dv_f, dcat_f] + vec_f, [dv_d, dcat_d] + vec_d):
            assert torch.equal(f_, d_), f"fused bwd with deferred finishes: {nm} differs from the undeferred launch"
        cat = lambda ts: torch.cat([t.detach() for t in ts], 3)
        # dv: the oracle stores the re-weighting's backward (radix*s*dout + dg) in bf16 before the norm backward; both product paths form it in
        # fp32 registers, so each is compared with the oracle at the bar the UNFUSED launch needs, and with each other at the plain bar below
        want_dv = cat([g_of(rec.conv[c + "conv2"][1]) for c in cards])
        e_u = rel(dv_u[..., :grp.V], want_dv)
        check("fused bwd: dv (gradient at the grouped conv2 output)", dv_f[..., :grp.V], want_dv, max(2 * TOL, 1.1 * e_u), worst=bw)
        assert e_u < 1e-2, f"unfused dv vs the oracle: {e_u:.2e}"
        want_du = cat([g_of(rec.conv[c + "conv1"][1]) for c in cards])
        e_u1 = rel(dcat_u[..., :grp.U], want_du)
        check("fused bwd: du_raw (gradient at the grouped conv1 output)", dcat_f[..., :grp.U], want_du, max(2 * TOL, 1.1 * e_u1), worst=bw)
        assert e_u1 < 1e-2, f"unfused du_raw vs the oracle: {e_u1:.2e}"      # (behind dv and du, LayerNorm backward amplifies)
        check("fused bwd: dsc_raw (gradient at the shortcut conv output)", dcat_f[..., grp.Up:], g_of(rec.conv[pre + "convtmp_sc"][1]), worst=bw)
        assert grp.Vp == grp.V or dv_f[..., grp.V:].abs().max().item() == 0, "fused bwd: pad channels"
        assert grp.Up == grp.U or dcat_f[..., grp.U:grp.Up].abs().max().item() == 0, "fused bwd: pad channels"
        check("fused bwd vs unfused launches: dv", dv_f, dv_u, worst=bw)
        check("fused bwd vs unfused launches: dcat", dcat_f, dcat_u, worst=bw)
        for nm, f_, u_ in zip(("dgamma2", "dbeta2", "dbias2", "dgamma1", "dbeta1", "dbias1", "dgamma_sc", "dbeta_sc", "dbias_sc"), vec_f, vec_u):
            check(f"fused bwd vs unfused launches: {nm}", f_, u_, worst=bw)
        print(f"stage {stage} fused bwd:", [(f"{e:.2e}", n) for e, n in sorted(bw, reverse=True)[:6]])
    print(f"stage {stage} worst:", [(f"{e:.2e}", n) for e, n in sorted(worst, reverse=True)[:5]])


def test_patch_embedding_and_decoder_layer_by_layer(world):
    from ultrasound_modeling_amd import ops
    net, P, rec = world
    dec = net.decoder
    worst = []
    conv_layer_check(net, rec, P, "transformer.embeddings.patch_embeddings", net.transformer.embeddings.patch_embeddings, worst)
    conv_layer_check(net, rec, P, "decoder.conv_more", dec.conv_more, worst)
    norm_layer_check(net, rec, P, "decoder.bn1", dec.bn1, worst, "ln")
    for i, blk in enumerate(dec.blocks):
        pre = f"decoder.blocks.{i}."
        oc, q = blk.out_channels, blk.out_channels // 4
        conv_layer_check(net, rec, P, pre + "up", blk.up, worst, transposed=True)                    # Decoder.py:63
        blk._fold = blk.conv1_0.fold_scale() is not None          # the mode the model runs (USSEG_FOLD_BN, default on)
        for stg in ("1", "2"):
            names = [f"{pre}conv{stg}_{j}" for j in range(4)]
            x = rec.conv[names[0]][0].detach()
            B, H, W, cin = x.shape
            xl, = fresh(x)
            lv = [fresh(P[n + ".kernel"], P[n + ".bias"]) for n in names]
            refs = [O.conv2d_same(xl, w, b, dl) for (w, b), dl in zip(lv, (1, 2, 4, 8))]
            xd = dev(x)
            raw = ops.new_act(B, H, W, oc, DEV)
            blk._branches_fwd(stg, xd, raw)                                                          # 1x1 + three dilated 3x3 in one multi-job launch
            if blk._fold:      # the launch already holds BatchNorm + LeakyReLU (scale in the packed operand, shift as the bias)
                bnn = [f"{pre}bn{stg}_{j}" for j in range(4)]
                fused = O.leaky_relu(torch.cat([O.batch_norm(r_, P[n + ".gamma"], P[n + ".beta"], P[n + ".moving_mean"], P[n + ".moving_variance"])
                                                for r_, n in zip(refs, bnn)], 3))
                want = torch.cat([folded_reference(x, P, cn, bn_, dl) for cn, bn_, dl in zip(names, bnn, (1, 2, 4, 8))], 3)
                check(f"{pre}stage{stg} branches+bn+act fwd (folded)", raw, bf(want), worst=worst)
                check(f"{pre}stage{stg} branches+bn+act fwd (folded) vs the unfolded fp64 composite", raw, bf(fused), 5 * TOL, worst=worst)
            else:
                check(f"{pre}stage{stg} branches fwd", raw, bf(torch.cat(refs, 3)), worst=worst)
            dys = [g_of(rec.conv[n][1]) for n in names]
            grads = torch.autograd.grad(refs, [xl] + [t for l in lv for t in l], dys)
            net.flat.zero_grad()
            dxd = ops.new_act(B, H, W, cin, DEV)
            with ops.overlap_region():
                blk._branches_bwd(stg, dev(torch.cat(dys, 3)), dxd)                                  # fused four-branch dgrad + multi-job wgrad
            torch.cuda.synchronize()
            check(f"{pre}stage{stg} fused dgrad", dxd, bf(grads[0]), worst=worst)
            for j, n in enumerate(names):
                check(f"{n} wgrad", getattr(blk, f"conv{stg}_{j}").kernel.grad, grads[1 + 2 * j], worst=worst)
            # the four BatchNorms + LeakyReLU as one launch (Decoder.py:68-76); dbias = the conv bias gradients
            bns = [f"{pre}bn{stg}_{j}" for j in range(4)]
            xs = [rec.norm[n][0].detach() for n in bns]
            nl = [fresh(xq, P[n + ".gamma"], P[n + ".beta"]) for xq, n in zip(xs, bns)]
            pre_act = torch.cat([O.batch_norm(xq, gq, bq, P[n + ".moving_mean"], P[n + ".moving_variance"]) for (xq, gq, bq), n in zip(nl, bns)], 3)
            ref = O.leaky_relu(pre_act)
            rawd = dev(torch.cat(xs, 3))
            if blk._fold:
                rawd = dev(bf(ref))        # mode 2 backward starts from the ACTIVATED tensor the folded forward stored
            else:
                act = blk._bn_fwd(stg, rawd, ops.new_act(B, H, W, oc, DEV))
                check(f"{pre}bn{stg} fwd", act, bf(ref), worst=worst)
            # the gradient arriving at the activated, concatenated tensor (Decoder.py:75-76)
            dy = g_of(rec.act_after(torch.cat([rec.norm[n][1] for n in bns], 3)))
            gr = torch.autograd.grad(ref, [t for l in nl for t in l], dy)
            net.flat.zero_grad()
            with ops.overlap_region():
                draw = blk._bn_bwd(stg, rawd, dev(dy), ops.new_act(B, H, W, oc, DEV))
            torch.cuda.synchronize()
            tol = 2 * TOL if blk._fold else TOL     # folded: xhat is rebuilt from the bf16 activation instead of read from the pre-norm tensor
            check(f"{pre}bn{stg} dx", draw, bf(torch.cat(gr[0::3], 3)), tol, worst=worst)
            for j in range(4):
                bn, cv = getattr(blk, f"bn{stg}_{j}"), getattr(blk, f"conv{stg}_{j}")
                check(f"{bns[j]} dgamma", bn.gamma.grad, gr[3 * j + 1], tol, worst=worst)
                check(f"{bns[j]} dbeta", bn.beta.grad, gr[3 * j + 2], tol, worst=worst)
                check(f"{pre}conv{stg}_{j} dbias", cv.bias.grad, gr[3 * j].sum(dim=(0, 1, 2)), tol, worst=worst)
    # ---- head: Conv2DTranspose(3x3, s2) + softmax (Decoder.py:120-121,142) in quad form, fused softmax + CCE loss, and back
    name = "decoder.head"
    x, y_logits, _ = rec.conv[name]
    x = x.detach()
    xl, wl, bl = fresh(x, P[name + ".kernel"], P[name + ".bias"])
    logits_ref = O.conv2d_transpose_s2_same(xl, wl, bl)
    B, h, w, _ = x.shape
    logits = dec._quad.forward(dev(x))                                                               # fp32 [B,h,w,16]: slot 4*(2a+b)+class
    full = logits.view(B, h, w, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, 4)
    check("head logits", full[..., :3], logits_ref, worst=worst)
    lg = full[..., :3].double().cpu().requires_grad_(True)                                           # the loss kernel on the product's own fp32 logits
    loss_ref = O.compute_loss(rec.y, O.softmax_lastaxis(lg), 2)
    loss_ref.backward()
    probs = torch.empty((B, 2 * h, 2 * w, 3), dtype=torch.float32, device=DEV)
    loss = torch.zeros(ops.ACC_FLOATS, dtype=torch.float32, device=DEV)
    dl4 = ops.new_act(B, h, w, 16, DEV, zero=True)
    ops.softmax_loss(logits, rec.y.float().to(DEV), probs, loss, dl4, HW=4 * h * w, C_classes=3, loss_kind=0, label_smoothing=0.1, clip_eps=1e-7,
                     inv_global_batch=0.5, quad_w=2 * w)
    check("softmax probs", probs, O.softmax_lastaxis(lg.detach()), worst=worst)
    assert abs(loss[0].item() - loss_ref.item()) < 1e-5 * abs(loss_ref.item())
    dfull = dl4.view(B, h, w, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * w, 4)
    check("softmax+CCE dlogits", dfull[..., :3], bf(lg.grad), worst=worst)
    dy = bf(dfull[..., :3].double().cpu())                                                           # head backward on the product's own bf16 dlogits
    gx, gw, gb = torch.autograd.grad(logits_ref, [xl, wl, bl], dy)
    net.flat.zero_grad()
    with ops.overlap_region():
        dx = dec._quad.backward(dl4)
    torch.cuda.synchronize()
    check("head dgrad", dx[..., :x.shape[-1]], bf(gx), worst=worst)
    check("head wgrad", dec.head.kernel.grad, gw, worst=worst)
    check("head dbias", dec.head.bias.grad, gb, worst=worst)
    print("decoder worst:", [(f"{e:.2e}", n) for e, n in sorted(worst, reverse=True)[:6]])
