"""tests/swin_restatement.py (the hand-written fp64 stages tests/test_gpu_swin_blocks.py holds the Swin encoder's launches to) against
oracle/swin_oracle.py, on the CPU: every composed tensor and all parameter gradients of block_ref / merge_ref / the whole chained model
equal torch.autograd.grad through S.swin_block / S.patch_merging / S.swin_forward to fp64 rounding (the bar of
test_cpu_fused_restatement.py), for the configuration the GPU file runs and its 'ape' and 'top' variants, with the stage outputs among
the differentiated outputs.  The hand-written LayerNorm is also held to route_probe.norm_ref / ln_wide_ref, whose references and
magnitudes the GPU file uses.

Two conditions on the GPU file's inputs are checked here, in fp64:
  1. for every stage-0 and stage-1 parameter the gradient caused by d_features alone is at least as large (L2) as the one caused by d_out
     alone, so a dropped d_features term is a relative error above one half in each of them (stage 1's PatchMerging is downstream of
     both stage outputs: d_features cannot reach it, which is asserted instead);
  2. no magnitude tensor that bounds a bf16 stage output or an fp32 sum is zero anywhere (no element's bound collapses to `tiny`).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import swin_oracle as S
import swin_restatement as R
from route_probe import ln_wide_ref, norm_ref, window_ref

TOL = 1e-12


def close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), (what, err)


def tok(t):
    return t.reshape(t.shape[0], -1, t.shape[-1])


_CACHE = {}


def model(variant):
    """The oracle's outputs and gradients (autograd, stage outputs differentiated with dfs) and model_ref's, once per variant."""
    if variant not in _CACHE:
        P = R.make_params(variant)
        x, d_out, dfs = R.make_inputs(variant)
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        out, feats = S.swin_forward(x, leaves, R.cfg_of(variant))
        both = torch.autograd.grad([out] + feats, list(leaves.values()), [d_out] + dfs, retain_graph=True)
        only_out = torch.autograd.grad(out, list(leaves.values()), d_out, retain_graph=True, allow_unused=True)
        _CACHE[variant] = dict(P=P, x=x, d_out=d_out, dfs=dfs, out=out.detach(), feats=[f.detach() for f in feats], grads=dict(zip(leaves, both)),
                               g_out=dict(zip(leaves, only_out)), ref=R.model_ref(x, d_out, dfs, P, variant))
    return _CACHE[variant]


@pytest.mark.parametrize("res,ws,shift,heads,C", [((8, 16), 4, 2, 2, 16), ((8, 8), 8, 0, 2, 16), ((4, 8), 4, 0, 1, 8)])
@pytest.mark.parametrize("done", [False, True])
def test_block_ref_against_oracle_autograd(res, ws, shift, heads, C, done):
    g = torch.Generator().manual_seed(C + shift)
    cfg = dict(patch_size=4, embed_dim=C, depths=[1], num_heads=[heads], window_size=ws)
    P = R.sub({k: v for k, v in S.init_swin_params(cfg, seed=3).items()}, "layers0/blocks0/")
    assert set(P) == set(R.BLOCK_PARAMS)
    x = torch.randn(2, *res, C, generator=g, dtype=torch.float64)
    dy = torch.randn(2, *res, C, generator=g, dtype=torch.float64)
    r = R.block_ref(x, dy, P, res, ws, shift, heads, incoming_bias_done=done)
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xl = x.clone().requires_grad_(True)
    y = S.swin_block(tok(xl), leaves, "", res, ws, shift, heads)
    grads = torch.autograd.grad(y, [xl] + list(leaves.values()), tok(dy))
    close(tok(r["y"]), y.detach(), "y")
    close(r["dx"], grads[0], "dx")
    for k, gr in zip(leaves, grads[1:]):
        close(r["grads"][k], gr, k)
    # the handoff table: the gradient values do not depend on who sums a bias, the flags do
    assert r["skip_bias"] == {"mlp/fc2": done, "mlp/fc1": True, "attn/proj": True, "attn/qkv": False}
    # intermediate tensors against their definitions in the oracle's terms
    n1 = S.layer_norm(x, P["norm1/gamma"], P["norm1/beta"])
    close(r["n1"], n1, "n1")
    close(r["qkv"], n1 @ P["attn/qkv/kernel"] + P["attn/qkv/bias"], "qkv")
    close(r["g"], S.gelu(r["h"]), "gelu")
    close(r["y"], r["a"] + r["g"] @ P["mlp/fc2/kernel"] + P["mlp/fc2/bias"], "y from a")
    hl = r["h"].clone().requires_grad_(True)
    close(R.gelu_d(r["h"]), torch.autograd.grad(S.gelu(hl).sum(), hl)[0], "gelu'")


def test_merge_embed_tail_against_oracle_autograd():
    g = torch.Generator().manual_seed(9)
    cfg = dict(patch_size=4, embed_dim=8, depths=[1, 1], num_heads=[1, 1], window_size=4, img_size=(16, 24), ape=True, include_top=True, num_classes=5)
    P = S.init_swin_params(cfg, in_chans=3, seed=4)
    x = torch.randn(2, 4, 6, 8, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 2, 3, 16, generator=g, dtype=torch.float64)
    r = R.merge_ref(x, dy, R.sub(P, "layers0/downsample/"))
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items() if k.startswith("layers0/downsample/")}
    xl = x.clone().requires_grad_(True)
    y = S.patch_merging(tok(xl), leaves, "layers0/", (4, 6))
    grads = torch.autograd.grad(y, [xl] + list(leaves.values()), tok(dy))
    close(tok(r["y"]), y.detach(), "merge y")
    close(r["dx"], grads[0], "merge dx")
    for k, gr in zip(leaves, grads[1:]):
        close(r["grads"][k[len("layers0/downsample/"):]], gr, k)
    close(R.patch_unmerge(R.patch_merge(x)), x, "unmerge(merge)")
    # token mean and its backward
    t = torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64)
    tl = t.clone().requires_grad_(True)
    d = torch.randn(2, 8, generator=g, dtype=torch.float64)
    close(R.token_mean(t)[0], tok(t).mean(1), "token mean")
    close(R.token_mean_bwd(d, t), torch.autograd.grad(tok(tl).mean(1), tl, d)[0], "token mean backward")
    # patchify + Dense == the strided convolution of the oracle
    img = torch.randn(2, 16, 24, 3, generator=g, dtype=torch.float64)
    w = P["patch_embed/proj/kernel"]
    want = torch.nn.functional.conv2d(img.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), P["patch_embed/proj/bias"], stride=4).permute(0, 2, 3, 1)
    close(R.dense(R.patchify(img, 4), w.reshape(-1, 8), P["patch_embed/proj/bias"])[0], want, "patch embedding")


def test_layer_norm_against_route_probe():
    g = torch.Generator().manual_seed(2)
    for C in (96, 768):
        x = torch.randn(37, C, generator=g, dtype=torch.float64) * 1.3 + 0.2
        dy = torch.randn(37, C, generator=g, dtype=torch.float64)
        gam, bet = 1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64), 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
        y, xh, rstd = R.layer_norm(x, gam, bet)
        dx, dg, db = R.layer_norm_bwd(xh, rstd, gam, dy)
        for r in (norm_ref(x, gam, bet, "none", dy=dy, eps=R.LN_EPS), ln_wide_ref(x, dy, gam, bet)):
            for got, key in ((y, "y"), (dx, "dx"), (dg, "dgamma"), (db, "dbeta")):
                close(got, r[key], f"C{C} {key}")


@pytest.mark.parametrize("variant", ["plain", "ape", "top"])
def test_model_ref_against_oracle_autograd(variant):
    m = model(variant)
    ref = m["ref"]
    close(ref["out"], m["out"], "out")
    for i, f in enumerate(m["feats"]):
        close(tok(ref["feats"][i]), f, f"feature {i}")
    assert set(ref["grads"]) == set(m["grads"])
    for k, gr in m["grads"].items():
        close(ref["grads"][k].reshape(gr.shape), gr, k)
    # the handoff flags of the chained model: a block's fc2 bias is summed upstream unless it is the last block of its stage
    for (s, i), b in ref["blocks"].items():
        assert b["skip_bias"]["mlp/fc2"] == (i < R.CFG["depths"][s] - 1)
    assert any(i not in (0, R.CFG["depths"][s] - 1) for s, i in ref["blocks"]), "the configuration must hold a middle block"


def test_condition_d_features_dominate_stage0_and_stage1_gradients():
    m = model("plain")
    worst = None
    for k, both in m["grads"].items():
        # every parameter d_features reaches: the blocks of stages 0 and 1 and stage 0's PatchMerging (through df1); stage 1's
        # PatchMerging lies behind both stage outputs, so no stage-output gradient enters it (asserted instead)
        if not k.startswith(("layers0/", "layers1/blocks")):
            if k.startswith("layers1/downsample/"):
                assert torch.equal(both, m["g_out"][k]), k
            continue
        g_out = m["g_out"][k]
        g_df = both - g_out                       # the backward pass is linear in its upstream gradients
        ratio = g_df.norm().item() / max(g_out.norm().item(), 1e-300)
        worst = min(worst, (ratio, k)) if worst else (ratio, k)
        assert g_df.norm().item() >= g_out.norm().item(), (k, ratio)
    print(f"\n  smallest |grad from d_features| / |grad from d_out|: {worst[0]:.2f} at {worst[1]}", end="")


def test_condition_no_zero_magnitude():
    """The mags the GPU file bounds with, evaluated on the unrounded fp64 chain of the same inputs: none is zero anywhere."""
    m = model("plain")
    P, ref = m["P"], m["ref"]
    heads, ws = R.CFG["num_heads"], R.CFG["window_size"]

    def positive(t, what):
        assert (t > 0).all(), f"{what}: {int((t <= 0).sum())} zero magnitudes"

    def ln_mags(x, dy, gam, bet, what, wide=False):
        C = x.shape[-1]
        r = ln_wide_ref(x.reshape(-1, C), dy.reshape(-1, C), gam, bet) if wide else norm_ref(x.reshape(-1, C), gam, bet, "none", dy=dy.reshape(-1, C), eps=R.LN_EPS)
        for key in ("ymag", "dxmag", "dgmag", "dbmag"):
            positive(r[key], f"{what} {key}")
    for (s, i), b in ref["blocks"].items():
        p = R.sub(P, f"layers{s}/blocks{i}/")
        what = f"stage {s} block {i}"
        ln_mags(b["x"], b["dn1"], p["norm1/gamma"], p["norm1/beta"], what + " norm1")
        ln_mags(b["a"], b["dn2"], p["norm2/gamma"], p["norm2/beta"], what + " norm2")
        for nm, xx, w, bias, dy in (("qkv", b["n1"], "attn/qkv", True, b["dqkv"]), ("proj", b["ctx"], "attn/proj", True, b["da"]),
                                    ("fc1", b["n2"], "mlp/fc1", True, b["dh"]), ("fc2", b["g"], "mlp/fc2", True, b["dy"])):
            positive(R.dense(xx, p[w + "/kernel"], p[w + "/bias"])[1], f"{what} {nm} forward")
            bw = R.dense_bwd(xx, p[w + "/kernel"], dy)
            for key in ("dxm", "dwm", "dbm"):
                positive(bw[key], f"{what} {nm} {key}")
        positive(b["g"].abs(), what + " gelu")
        positive(b["dh"].abs(), what + " gelu backward")
        wsz, shift = S.block_window(R.stage_res(s), ws, i)
        wr = window_ref(b["qkv"], b["dctx"], p["attn/relative_position_bias_table"], heads[s], wsz, shift, list(range(R.BATCH)))
        for key in ("om", "dqkvm", "dtablem"):
            positive(wr[key], f"{what} window {key}")
    for s, mr in ref["merges"].items():
        p = R.sub(P, f"layers{s}/downsample/")
        ln_mags(mr["m"], mr["dn"], p["norm/gamma"], p["norm/beta"], f"merge {s} norm", wide=mr["m"].shape[-1] > 512)
        positive(R.dense(mr["n"], p["reduction/kernel"])[1], f"merge {s} reduction")
    t = ref["tail"]
    positive(R.token_mean(t["n"])[1], "token mean")
    positive(t["dn"].abs(), "token mean backward")
