"""fp64 restatement of the windowed-attention encoder (ultrasound_modeling_amd/SwinTransformer.py) stage by stage, forward AND backward,
written out by hand - no autograd in any backward here.  It imports nothing from the product: tests/test_cpu_swin_blocks.py pins it to
oracle/swin_oracle.py (torch.autograd.grad through S.swin_block / S.patch_merging / S.swin_forward, fp64 rounding), and
tests/test_gpu_swin_blocks.py holds every launch of the product's forward and backward pass to it, from the product's own stored input
to that launch.

Tokens are [B, H, W, C] (the oracle's [B, L = H*W, C] row-major).  Every stage function returns its result AND its magnitude: the same
operation on absolute values, which is what route_probe.acheck / assert_elementwise scale a bound with.  The windowed attention, the
packed LayerNorm and the wide LayerNorm take their per-element references and magnitudes from route_probe (window_ref, norm_ref,
ln_wide_ref); the LayerNorm written out here is what the composed references use, and the CPU file checks it against those.

Composed references: block_ref, merge_ref, embed_ref, tail_ref.  CFG / make_inputs are the one configuration both test files run:
(64, 128) image, patch 4, embed 96, depths [3, 2, 2], heads [3, 6, 12], window 8, batch 2 - token grids 16x32 (8x8 windows, head size
32, shift 0 and 4, a middle block, merge LayerNorm at 384), 8x16 (one-window rule, merge LayerNorm at 768: the wide kernel) and 4x8
(window 4).  DF_SCALE scales the stage-output gradients so that, for every stage-0 and stage-1 parameter, the gradient they cause alone
is at least as large as the one d_out causes alone (checked in fp64 by the CPU file): a dropped d_features term then costs more than
half of each of those gradients and cannot hide inside a relative-L2 bar.
"""
import math

import torch

import swin_oracle as S
from route_probe import window_ref

LN_EPS = S.LN_EPS
CFG = dict(img_size=(64, 128), patch_size=4, in_chans=1, embed_dim=96, depths=[3, 2, 2], num_heads=[3, 6, 12], window_size=8)
BATCH = 2
NUM_CLASSES = 10
DF_SCALE = 1.0
BLOCK_PARAMS = ("norm1/gamma", "norm1/beta", "attn/qkv/kernel", "attn/qkv/bias", "attn/relative_position_bias_table", "attn/proj/kernel",
                "attn/proj/bias", "norm2/gamma", "norm2/beta", "mlp/fc1/kernel", "mlp/fc1/bias", "mlp/fc2/kernel", "mlp/fc2/bias")


def bf(t):
    return t.detach().to(torch.bfloat16).to(torch.float64)


def cfg_of(variant="plain"):
    """The oracle's configuration dict of a variant: 'plain', 'ape' (absolute position embedding) or 'top' (classification head)."""
    c = dict(CFG, ape=variant == "ape", include_top=variant == "top")
    if variant == "top":
        c["num_classes"] = NUM_CLASSES
    return c


def make_params(variant="plain", seed=5):
    """S.init_swin_params(perturb=True): kernels rounded to bf16-representable values (the product's GEMM operands ARE the bf16 rounding of
    its fp32 masters, so this takes the operand rounding out of both sides), every other parameter arbitrary fp32.  A stage under the
    one-window rule (SwinTransformer.py:172-175) builds its attention with the reduced window, so its bias table has (2*window - 1)^2 rows:
    the rows of the oracle's table that its relative_position_index reaches."""
    P = S.init_swin_params(cfg_of(variant), in_chans=CFG["in_chans"], seed=seed, perturb=True)
    P = {k: (bf(v) if k.endswith("/kernel") else v.float().double()) for k, v in P.items()}
    for s, depth in enumerate(CFG["depths"]):
        for i in range(depth):
            wsz, _ = S.block_window(stage_res(s), CFG["window_size"], i)
            k = f"layers{s}/blocks{i}/attn/relative_position_bias_table"
            P[k] = P[k][:(2 * wsz - 1) ** 2].clone()
    return P


def make_inputs(variant="plain", seed=6):
    """bf16-representable image and stage-output gradients, fp32 d_out: -> x [B,H,W,1], d_out [B,F or classes], [df0, df1] as [B,L,C]."""
    g = torch.Generator().manual_seed(seed)
    H, W = CFG["img_size"]
    ps, E = CFG["patch_size"], CFG["embed_dim"]
    x = bf(torch.randn(BATCH, H, W, CFG["in_chans"], generator=g, dtype=torch.float64))
    nout = NUM_CLASSES if variant == "top" else E * 2 ** (len(CFG["depths"]) - 1)
    d_out = torch.randn(BATCH, nout, generator=g, dtype=torch.float64).float().double()
    dfs = [bf(DF_SCALE * torch.randn(BATCH, (H // ps >> i) * (W // ps >> i), E << i, generator=g, dtype=torch.float64))
           for i in range(len(CFG["depths"]) - 1)]
    return x, d_out, dfs


def stage_res(i):
    H, W = CFG["img_size"]
    return (H // CFG["patch_size"]) >> i, (W // CFG["patch_size"]) >> i


# ------------------------------------------------------------------------------------------------ stages
def dense(x, w, b=None, res=None):
    """y = x @ w + b (+ res) over the last axis: -> (y, mag)."""
    y, m = x @ w, x.abs() @ w.abs()
    if b is not None:
        y, m = y + b, m + b.abs()
    if res is not None:
        y, m = y + res, m + res.abs()
    return y, m


def dense_bwd(x, w, dy):
    """-> dict(dx = dy @ w^T, dw = x^T @ dy, db = column sums of dy) and the mags dxm, dwm, dbm (sums of absolute terms)."""
    x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    return dict(dx=dy @ w.T, dxm=dy.abs() @ w.abs().T, dw=x2.T @ dy2, dwm=x2.abs().T @ dy2.abs(), db=dy2.sum(0), dbm=dy2.abs().sum(0))


def colsum(t):
    """-> (column sums over the tokens, the sums of absolute terms)."""
    t2 = t.reshape(-1, t.shape[-1])
    return t2.sum(0), t2.abs().sum(0)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_d(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def layer_norm(x, g, b):
    """-> (y, xhat, rstd) over the last axis, eps = LN_EPS."""
    mu = x.mean(-1, keepdim=True)
    rstd = (((x - mu) ** 2).mean(-1, keepdim=True) + LN_EPS).rsqrt()
    xh = (x - mu) * rstd
    return xh * g + b, xh, rstd


def layer_norm_bwd(xh, rstd, g, dy):
    """-> (dx, dgamma, dbeta): dx = rstd*(g*dy - mean(g*dy) - xhat*mean(g*dy*xhat))."""
    t = dy * g
    dx = rstd * (t - t.mean(-1, keepdim=True) - xh * (t * xh).mean(-1, keepdim=True))
    C = xh.shape[-1]
    return dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)


def add(a, b):
    return a + b, a.abs() + b.abs()


def patch_merge(x):
    """[B,H,W,C] -> [B,H/2,W/2,4C] in the reference's order x0=(0,0), x1=(1,0), x2=(0,1), x3=(1,1) (SwinTransformer.py:280-284)."""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


def patch_unmerge(m):
    B, H2, W2, C4 = m.shape
    C = C4 // 4
    x = torch.zeros(B, 2 * H2, 2 * W2, C, dtype=m.dtype, device=m.device)
    x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2] = m[..., :C], m[..., C:2 * C], m[..., 2 * C:3 * C], m[..., 3 * C:]
    return x


def patchify(img, ps):
    """[B,H,W,Cin] -> [B,H/ps,W/ps,ps*ps*Cin], channel order (row in patch, column in patch, channel): Conv2D(kernel = stride = ps) is then
    a Dense layer with the Keras kernel [ps,ps,Cin,E] read as [ps*ps*Cin, E]."""
    B, H, W, C = img.shape
    return img.reshape(B, H // ps, ps, W // ps, ps, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // ps, W // ps, ps * ps * C)


def token_mean(x):
    """[B,H,W,C] -> ([B,C] mean over the tokens, the mean of |x|)."""
    return x.mean((1, 2)), x.abs().mean((1, 2))


def token_mean_bwd(dy, like):
    B, H, W, C = like.shape
    return (dy / (H * W))[:, None, None, :].expand(B, H, W, C)


# ------------------------------------------------------------------------------------------------ composed references
def skip_bias(incoming_bias_done):
    """Which Dense backward of a block must NOT sum its bias gradient, because another launch does: fc1 (the GELU backward sums dh), proj
    (norm2's backward + residual sums da), fc2 only when the launch that produced the block's dy already summed it into fc2.bias.grad."""
    return {"mlp/fc2": bool(incoming_bias_done), "mlp/fc1": True, "attn/proj": True, "attn/qkv": False}


def block_ref(x, dy, P, res, ws, shift, heads, incoming_bias_done=False):
    """One SwinTransformerBlock (SwinTransformer.py:219-261) forward from x [B,H,W,C] and backward from dy, without any rounding.  P maps
    the 13 names of BLOCK_PARAMS to fp64 tensors.  Returns every intermediate tensor by the product's names
      forward:  x, n1, qkv, ctx, a (= x + proj(ctx)), n2, h, g (= gelu(h)), y (= a + fc2(g))
      backward: dy, dg, dh, dn2, da (= LN2'(dn2) + dy), dctx, dqkv, dn1, dx (= LN1'(dn1) + da)
    the 13 parameter gradients under 'grads', and under 'skip_bias' which Dense backward must NOT sum its bias gradient because another
    launch does: fc1 (act_bwd_colsum sums dh), proj (norm2's backward_residual sums da), fc2 only when the kernel that produced dy already
    summed it (`incoming_bias_done`: the block above handed this block's fc2.bias.grad to its norm1 backward_residual)."""
    H, W = res
    B = x.shape[0]
    assert tuple(x.shape[1:3]) == (H, W)
    keep = list(range(B))
    r = {"x": x, "dy": dy}
    r["n1"], xh1, rstd1 = layer_norm(x, P["norm1/gamma"], P["norm1/beta"])
    r["qkv"], _ = dense(r["n1"], P["attn/qkv/kernel"], P["attn/qkv/bias"])
    table = P["attn/relative_position_bias_table"]
    r["ctx"] = window_ref(r["qkv"], torch.zeros_like(x), table, heads, ws, shift, keep)["o"]
    r["a"], _ = dense(r["ctx"], P["attn/proj/kernel"], P["attn/proj/bias"], x)
    r["n2"], xh2, rstd2 = layer_norm(r["a"], P["norm2/gamma"], P["norm2/beta"])
    r["h"], _ = dense(r["n2"], P["mlp/fc1/kernel"], P["mlp/fc1/bias"])
    r["g"] = gelu(r["h"])
    r["y"], _ = dense(r["g"], P["mlp/fc2/kernel"], P["mlp/fc2/bias"], r["a"])
    G = {}
    fc2 = dense_bwd(r["g"], P["mlp/fc2/kernel"], dy)
    r["dg"], G["mlp/fc2/kernel"], G["mlp/fc2/bias"] = fc2["dx"], fc2["dw"], fc2["db"]
    r["dh"] = r["dg"] * gelu_d(r["h"])
    fc1 = dense_bwd(r["n2"], P["mlp/fc1/kernel"], r["dh"])
    r["dn2"], G["mlp/fc1/kernel"], G["mlp/fc1/bias"] = fc1["dx"], fc1["dw"], fc1["db"]
    d2, G["norm2/gamma"], G["norm2/beta"] = layer_norm_bwd(xh2, rstd2, P["norm2/gamma"], r["dn2"])
    r["da"], _ = add(d2, dy)
    proj = dense_bwd(r["ctx"], P["attn/proj/kernel"], r["da"])
    r["dctx"], G["attn/proj/kernel"], G["attn/proj/bias"] = proj["dx"], proj["dw"], proj["db"]
    wr = window_ref(r["qkv"], r["dctx"], table, heads, ws, shift, keep)
    r["dqkv"], G["attn/relative_position_bias_table"] = wr["dqkv"], wr["dtable"]
    qkv = dense_bwd(r["n1"], P["attn/qkv/kernel"], r["dqkv"])
    r["dn1"], G["attn/qkv/kernel"], G["attn/qkv/bias"] = qkv["dx"], qkv["dw"], qkv["db"]
    d1, G["norm1/gamma"], G["norm1/beta"] = layer_norm_bwd(xh1, rstd1, P["norm1/gamma"], r["dn1"])
    r["dx"], _ = add(d1, r["da"])
    assert set(G) == set(BLOCK_PARAMS)
    r["grads"] = G
    r["skip_bias"] = skip_bias(incoming_bias_done)
    return r


def merge_ref(x, dy, P):
    """PatchMerging (SwinTransformer.py:264-290): P = {'norm/gamma', 'norm/beta', 'reduction/kernel'}; -> m, n, y, dn, dm, dx, grads."""
    r = {"m": patch_merge(x)}
    r["n"], xh, rstd = layer_norm(r["m"], P["norm/gamma"], P["norm/beta"])
    r["y"], _ = dense(r["n"], P["reduction/kernel"])
    red = dense_bwd(r["n"], P["reduction/kernel"], dy)
    r["dn"] = red["dx"]
    r["dm"], dg, db = layer_norm_bwd(xh, rstd, P["norm/gamma"], r["dn"])
    r["dx"] = patch_unmerge(r["dm"])
    r["grads"] = {"reduction/kernel": red["dw"], "norm/gamma": dg, "norm/beta": db}
    return r


def embed_ref(img, dt, P, ps, ape=None):
    """PatchEmbed (+ the absolute position embedding [1,L,E], SwinTransformer.py:341-365,442-443) from the image, backward from dt, the
    gradient of the embedded tokens: P = {'proj/kernel' [ps,ps,Cin,E], 'proj/bias', 'norm/gamma', 'norm/beta'}; -> p, t, e, dtn, grads
    (with 'absolute_pos_embed' when ape is given: dt summed over the batch)."""
    r = {"p": patchify(img, ps)}
    w = P["proj/kernel"].reshape(-1, P["proj/kernel"].shape[-1])
    r["t"], _ = dense(r["p"], w, P["proj/bias"])
    r["e"], xh, rstd = layer_norm(r["t"], P["norm/gamma"], P["norm/beta"])
    G = {}
    if ape is not None:
        r["e"] = r["e"] + ape.reshape(1, *r["e"].shape[1:])
        G["absolute_pos_embed"] = dt.sum(0).reshape(ape.shape)
    r["dtn"], G["norm/gamma"], G["norm/beta"] = layer_norm_bwd(xh, rstd, P["norm/gamma"], dt)
    pr = dense_bwd(r["p"], w, r["dtn"])
    G["proj/kernel"], G["proj/bias"] = pr["dw"].reshape(P["proj/kernel"].shape), pr["db"]
    r["grads"] = G
    return r


def tail_ref(t, d_out, P, head=None):
    """Final LayerNorm, token mean and the optional head (SwinTransformer.py:450-455): P = {'norm/gamma', 'norm/beta'}, head =
    {'kernel', 'bias'} or None; -> n, pooled, out, dpooled, dn, dt, grads."""
    r = {}
    r["n"], xh, rstd = layer_norm(t, P["norm/gamma"], P["norm/beta"])
    r["pooled"], _ = token_mean(r["n"])
    G = {}
    if head is not None:
        r["out"], _ = dense(r["pooled"], head["kernel"], head["bias"])
        hb = dense_bwd(r["pooled"], head["kernel"], d_out)
        r["dpooled"], G["head/kernel"], G["head/bias"] = hb["dx"], hb["dw"], hb["db"]
    else:
        r["out"], r["dpooled"] = r["pooled"], d_out
    r["dn"] = token_mean_bwd(r["dpooled"], r["n"])
    r["dt"], G["norm/gamma"], G["norm/beta"] = layer_norm_bwd(xh, rstd, P["norm/gamma"], r["dn"])
    r["grads"] = G
    return r


def sub(P, prefix):
    """The parameters under `prefix` with the prefix removed."""
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def model_ref(x, d_out, dfs, P, variant="plain"):
    """The composed references chained over the whole model of CFG: the forward pass, then the backward pass with the stage-output
    gradients dfs added after each PatchMerging backward.  -> dict(out, feats, grads by the oracle's names, blocks = {(stage, i): block_ref
    result}, merges, embed, tail)."""
    depths, heads, ws, ps = CFG["depths"], CFG["num_heads"], CFG["window_size"], CFG["patch_size"]
    ns = len(depths)
    zero = lambda t: torch.zeros_like(t)
    # forward: every *_ref is linear in its upstream gradient, so the forward tensors do not depend on the dy handed in here
    ape = P.get("absolute_pos_embed")
    emb = embed_ref(x, torch.zeros(BATCH, *stage_res(0), CFG["embed_dim"], dtype=torch.float64), sub(P, "patch_embed/"), ps, ape)
    t, xin, feats = emb["e"], {}, []
    for s in range(ns):
        for i in range(depths[s]):
            xin[s, i] = t
            wsz, shift = S.block_window(stage_res(s), ws, i)
            t = block_ref(t, zero(t), sub(P, f"layers{s}/blocks{i}/"), stage_res(s), wsz, shift, heads[s])["y"]
        if s < ns - 1:
            feats.append(t)
            t = merge_ref(t, torch.zeros(BATCH, *stage_res(s + 1), 2 * t.shape[-1], dtype=torch.float64), sub(P, f"layers{s}/downsample/"))["y"]
    head = sub(P, "head/") if variant == "top" else None
    tail = tail_ref(t, d_out, {k: P[k] for k in ("norm/gamma", "norm/beta")}, head)
    G = dict(tail["grads"])
    d, blocks, merges = tail["dt"], {}, {}
    for s in reversed(range(ns)):
        if s < ns - 1:
            merges[s] = merge_ref(feats[s], d, sub(P, f"layers{s}/downsample/"))
            G.update({f"layers{s}/downsample/{k}": v for k, v in merges[s]["grads"].items()})
            d = merges[s]["dx"] + dfs[s].reshape(merges[s]["dx"].shape)
        for i in reversed(range(depths[s])):
            wsz, shift = S.block_window(stage_res(s), ws, i)
            blocks[s, i] = block_ref(xin[s, i], d, sub(P, f"layers{s}/blocks{i}/"), stage_res(s), wsz, shift, heads[s],
                                     incoming_bias_done=i < depths[s] - 1)
            G.update({f"layers{s}/blocks{i}/{k}": v for k, v in blocks[s, i]["grads"].items()})
            d = blocks[s, i]["dx"]
    emb = embed_ref(x, d, sub(P, "patch_embed/"), ps, ape)
    G.update({(k if k == "absolute_pos_embed" else "patch_embed/" + k): v for k, v in emb["grads"].items()})
    return dict(out=tail["out"], feats=feats, grads=G, blocks=blocks, merges=merges, embed=emb, tail=tail)
