"""The Swin encoder stage by stage IN the model (GPU): every launch of one forward and one backward pass of SwinTransformerModel, checked
from the product's own stored input to that launch, with every gradient handoff of the hand-built backward pass asserted.

One model (tests/swin_restatement.py CFG: (64, 128) image, patch 4, embed 96, depths [3, 2, 2], heads [3, 6, 12], window 8, batch 2) runs
forward(x) and backward(d_out, d_features=[df0, df1]) once under a recorder that wraps, for its duration, the ops.* functions and
Conv2D.forward / Conv2D.backward that SwinTransformer.py calls, and keeps a clone taken AT CALL TIME of every argument tensor, a clone
of every argument after the call (outputs written in place) and of every result, in call order - copy_channels(accumulate=True) later
mutates tensors that were already returned.  The recorder changes no behaviour.  Then, walking the recorded calls in the order the
architecture prescribes (a call out of place fails the walk):

  * each launch is recomputed in fp64 on the device from the inputs the product handed it, and every element is bounded with the
    constants of tests/route_probe.py - bf16 outputs: U_BF16, C_BOUND and the stage's magnitude (Dense: |x|.|W| + |b| + |residual|, the
    bound of test_gpu_conv_routes.py for a 1x1 conv; LayerNorm, wide LayerNorm and the windowed attention: norm_ref / ln_wide_ref /
    window_ref with their ext terms, as test_gpu_norm_routes.py and test_gpu_attn_routes.py; GELU, its backward, copy_channels(accumulate)
    and the token mean as test_gpu_pointwise_routes.py / test_gpu_attn_routes.py); fp32 sums over M tokens: U_F32, c_f32(M), mag = the sum
    of absolute terms.  Stages that round twice say so: the fused LayerNorm backward + residual stores bf16(bf16(LN'(dy)) + dres), c = 2 *
    C_BOUND (test_layernorm_backward_res); the unfused route is checked launch by launch with C_BOUND each, and as a whole against
    LN'(dy) + dres with 2 * C_BOUND - its second rounding is the accumulate.  patchify, patch_merge and the fp32 casts are bitwise.
    No element is left out of any check.
  * each launch's input must BE the tensor the restatement says it is: torch.equal with the recorded output of its producer (norm2's dres
    is the block's incoming dy, norm1's dres is da, the tensor merged back in stage i is downsample.backward(...) + df_i, ...), the
    parameter vectors and gradient destinations it was given must be the named parameter's, and every skip_bias flag must be the one
    swin_restatement.block_ref states.  This is what catches a mis-wired tensor that is numerically plausible.
  * every parameter gradient is checked exactly once, from flat.grad zeroed before the pass, against the fp64 sum of the recorded tensors
    that define it: fc2.bias.grad of block i = colsum(dy_i), proj.bias.grad = colsum(da), fc1.bias.grad = colsum(dh), qkv.bias.grad =
    colsum(dqkv), the relative-position table from window_ref, the LayerNorm gamma / beta, every kernel gradient x^T.dy,
    absolute_pos_embed.grad ('ape' variant), head.kernel.grad / head.bias.grad ('top' variant, 10 classes).  A gradient summed twice
    or never is off by about 100 %.  Every stand-alone colsum launch must be one the walk expects, on the tensor it expects.
  * the first launch of every route runs under route_probe.routed and must show its kernel: packed LayerNorm forward / backward /
    backward + residual (kname), ln_wide_kernel<2, *>, window_attn_mfma_kernel<*, true> and window_attn_kernel<*, 4>, act_fwd_kernel,
    act_bwd_colsum_kernel, copy_channels_kernel, colsum_kernel<0>, the token-mean kernels, reduce_finish_kernel behind the head's bias
    sum (it runs before the overlap region) and reduce_finish_batched_kernel at the end of the overlap region, where the deferred sums of
    the backward pass finish.

All four combinations of SwinTransformer._FUSE_LN_RES and SwinTransformer._LAZY_BLOCK run the stage checks; across _LAZY_BLOCK every
gradient is bit-identical.  The same runs are compared with S.swin_forward autograd (stage outputs among the differentiated outputs, [df0,
df1] their upstream gradients) at the relative-L2 bars of test_small_swin_model_against_the_oracle.  tests/test_cpu_swin_blocks.py holds
the restatement to the oracle and checks the two conditions on these inputs (d_features dominate the stage-0 / stage-1 gradients; no
magnitude is zero).  Each check prints its worst ratio err / bound (run with -s); test_zz_worst_ratio_table prints the worst per stage
kind and switch combination.  Measured on an MI355X (the same under all four switch settings; the bounds are route_probe's constants, not
fitted to these): Dense forward 0.22, backward-data 0.13 (head 0.20); LayerNorm forward 0.25, backward 0.21, backward + residual 0.15
fused and 0.15 unfused (0.17 with ape); wide LayerNorm 0.25 / 0.18; MFMA window 0.25 / 0.19 (0.20 with ape), generic window 0.25 / 0.25;
GELU 0.24 / 0.25; accumulate 0.25; token mean 0.007 / 0.24; gradients: kernels 0.06, biases 0.011, LayerNorm 0.027, table and ape below 0.001.
"""
import contextlib
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import swin_oracle as S
import swin_restatement as R
from route_probe import C_BOUND, U_BF16, U_F32, acheck, c_f32, kname, ln_wide_ref, norm_ref, routed, window_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
OPS = ("patchify", "norm_act_fwd", "ln_wide_fwd", "norm_act_bwd", "ln_wide_bwd", "norm_act_bwd_res", "copy_channels", "colsum", "act_fwd",
       "act_bwd_colsum", "window_attn_fwd", "window_attn_bwd", "patch_merge", "token_mean_fwd", "token_mean_bwd", "to_f32")
REGION_END = ("overlap_region end",)
WORST = {}       # (switches, stage kind) -> worst err / bound
_RUNS = {}
_ORACLE = {}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def eq(a, b, what):
    assert a is not None and b is not None, what
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ recorder
class Call:
    def __init__(self, name):
        self.name, self.mod, self.a, self.ptr, self.post, self.out = name, None, {}, {}, {}, None


class Recorder:
    """Wraps ops.<OPS> and Conv2D.forward / Conv2D.backward while the block runs; calls are kept in the order they were entered."""

    def __init__(self, net, routes):
        self.calls = []
        self.mods = {id(m): n for n, m in net.named_modules()}
        self.routes, self.seen = routes, {}

    def _wrap(self, name, fn, conv=False):
        sig, rec = inspect.signature(fn), self

        def wrapped(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            c = Call(name)
            for n, v in ba.arguments.items():
                if n == "self":
                    continue
                c.a[n] = v.clone() if torch.is_tensor(v) else v
                if torch.is_tensor(v):
                    c.ptr[n] = v.data_ptr()
            if conv:
                layer = ba.arguments["self"]
                c.mod = rec.mods[id(layer)]
                if name == "conv_bwd":
                    c.a["x"] = layer._x.clone()
            rec.calls.append(c)
            key = route_key(c)
            if key in rec.routes and key not in rec.seen:      # the first launch of each route runs under the kernel probe
                out, rec.seen[key] = routed(lambda: fn(*args, **kw), *rec.routes[key])
            else:
                out = fn(*args, **kw)
            c.post = {n: v.clone() for n, v in ba.arguments.items() if torch.is_tensor(v)}
            c.out = out.clone() if torch.is_tensor(out) else out
            return out
        return wrapped

    def _region(self, orig):
        """ops.overlap_region with its exit - where the deferred sums of the backward pass finish - under the kernel probe."""
        rec = self

        @contextlib.contextmanager
        def region():
            cm = orig()
            cm.__enter__()
            try:
                yield
            finally:
                _, rec.seen[REGION_END] = routed(lambda: cm.__exit__(None, None, None), *rec.routes[REGION_END])
        return region

    def __enter__(self):
        from ultrasound_modeling_amd import ops
        from ultrasound_modeling_amd.layers import Conv2D
        self._saved = ([(ops, n, getattr(ops, n)) for n in OPS + ("overlap_region",)]
                       + [(Conv2D, "forward", Conv2D.forward), (Conv2D, "backward", Conv2D.backward)])
        for n in OPS:
            setattr(ops, n, self._wrap(n, getattr(ops, n)))
        ops.overlap_region = self._region(ops.overlap_region)
        Conv2D.forward = self._wrap("conv_fwd", Conv2D.forward, conv=True)
        Conv2D.backward = self._wrap("conv_bwd", Conv2D.backward, conv=True)
        return self

    def __exit__(self, *exc):
        for owner, n, fn in self._saved:
            setattr(owner, n, fn)


class Cursor:
    def __init__(self, calls):
        self.calls, self.i = calls, 0

    def next(self, name):
        assert self.i < len(self.calls), f"the pass ended where a {name} call was expected"
        c = self.calls[self.i]
        assert c.name == name, f"call {self.i}: expected {name}, the product called {c.name} ({c.mod})"
        self.i += 1
        return c

    def done(self):
        assert self.i == len(self.calls), f"{len(self.calls) - self.i} calls after the expected end: {[c.name for c in self.calls[self.i:]]}"


# ------------------------------------------------------------------------------------------------ the run
def oname(k):
    """'basic_layers.0.blocks.1.attn.qkv' -> the oracle's 'layers0/blocks1/attn/qkv'."""
    return k.replace("basic_layers.", "layers").replace("blocks.", "blocks").replace(".", "/")


def name_map(net):
    return {k: oname(k) for k, _ in net.named_parameters()}


def route_key(c):
    """The route of a recorded call, as far as its arguments decide it: the op, and for the windowed attention its window and whether
    it is the MFMA kernel's shape (8x8 windows, head size 32).  Dense layers are not probed: test_gpu_conv_routes.py names their kernels."""
    if c.name in ("window_attn_fwd", "window_attn_bwd"):
        ws, d = c.a["ws"], c.a["qkv"].shape[-1] // 3 // c.a["heads"]
        return (c.name, ws, ws == 8 and d == 32)
    if c.name in ("conv_fwd", "conv_bwd"):
        return None
    return (c.name,)


def expected_routes(variant, fuse):
    """route_key -> the kernels its first launch must show.  With 8 windows (stage 0) or 2 (stage 1) per image, 3 or 6 heads and batch 2
    the MFMA window kernel stays below its multi-window floors: one window per workgroup, forward and backward."""
    r = {("norm_act_fwd",): [kname(False, 0, 1)], ("norm_act_bwd",): [kname(True, 0, 1)],
         ("ln_wide_fwd",): ["ln_wide_kernel<2, false>"], ("ln_wide_bwd",): ["ln_wide_kernel<2, true>"],
         ("window_attn_fwd", 8, True): ["window_attn_mfma_kernel<false, true>"], ("window_attn_bwd", 8, True): ["window_attn_mfma_kernel<true, true>"],
         ("window_attn_fwd", 4, False): ["window_attn_kernel<false, 4>"], ("window_attn_bwd", 4, False): ["window_attn_kernel<true, 4>"],
         ("act_fwd",): ["act_fwd_kernel"], ("act_bwd_colsum",): ["act_bwd_colsum_kernel"], ("copy_channels",): ["copy_channels_kernel"],
         ("colsum",): ["colsum_kernel<0>"], REGION_END: ["reduce_finish_batched_kernel"], ("token_mean_fwd",): ["token_mean_fwd_kernel"], ("token_mean_bwd",): ["token_mean_bwd_kernel"]}
    if fuse:
        r[("norm_act_bwd_res",)] = [kname(True, 0, 1, res=True)]
    if variant == "top":       # the first bias sum is the head's, before the overlap region: it finishes at once
        r[("colsum",)] = ["colsum_kernel<0>", "reduce_finish_kernel"]
    return r


def get_run(monkeypatch, variant, fuse, lazy):
    key = (variant, fuse, lazy)
    if key in _RUNS:
        return _RUNS[key]
    from ultrasound_modeling_amd import SwinTransformer as ST
    from ultrasound_modeling_amd import ops
    monkeypatch.setattr(ST, "_FUSE_LN_RES", 1 if fuse else 0)
    monkeypatch.setattr(ST, "_LAZY_BLOCK", 1 if lazy else 0)
    assert ops._LAZY, "lazy weight gradients are the default: _LAZY_BLOCK decides per block"
    c = R.CFG
    net = ST.SwinTransformerModel(model_name="blocks", include_top=variant == "top", num_classes=R.NUM_CLASSES, img_size=c["img_size"],
                                  patch_size=(c["patch_size"],) * 2, in_chans=c["in_chans"], embed_dim=c["embed_dim"], depths=c["depths"],
                                  num_heads=c["num_heads"], window_size=c["window_size"], ape=variant == "ape")
    P = R.make_params(variant)
    names = name_map(net)
    assert set(names.values()) == set(P)
    own = {names[k]: p for k, p in net.named_parameters()}
    for k, p in own.items():
        assert p.numel() == P[k].numel(), (k, tuple(p.shape), tuple(P[k].shape))
        p.data.copy_(P[k].float().reshape(p.shape))
    net.repack()
    x, d_out, dfs = R.make_inputs(variant)
    xd, dod, dfd = x.float().to(DEV), d_out.float().to(DEV), [f.to(BF16).to(DEV) for f in dfs]
    net.flat.zero_grad()
    torch.cuda.synchronize()
    routes = expected_routes(variant, fuse)
    with Recorder(net, routes) as rec:
        out, feats = net.forward(xd)
        feats = [f.clone() for f in feats]
        net.backward(dod, d_features=dfd)
    torch.cuda.synchronize()
    run = dict(net=net, own=own, calls=rec.calls, out=out.clone(), feats=feats, routes=routes, seen=rec.seen, grad=net.flat.grad.clone(), x=xd, d_out=dod, dfs=dfd,
               variant=variant, fuse=fuse, lazy=lazy, tag=f"{variant} fuse={int(fuse)} lazy={int(lazy)}")
    _RUNS[key] = run
    return run


# ------------------------------------------------------------------------------------------------ the walk
class Walk:
    def __init__(self, run):
        self.run, self.net, self.own, self.tag = run, run["net"], run["own"], run["tag"]
        self.mods = dict(self.net.named_modules())
        self.it = Cursor([c for c in run["calls"] if c.name != "colsum"])
        self.colsums = [c for c in run["calls"] if c.name == "colsum"]
        self.want_colsums = []       # (destination pointer, tensor) of every stand-alone colsum launch the walk expects
        self.expect = {}             # parameter name -> (reference, magnitude, summed terms, ext or None, kind)
        self.fw = {}
        self.win = {}

    # ---- bounds
    def note(self, kind, ratio):
        k = (self.tag, kind)
        WORST[k] = max(WORST.get(k, 0.0), ratio)

    def b16(self, kind, what, y, ref, mag, c=C_BOUND, extra=None):
        self.note(kind, acheck(f"{self.tag} {what}", y, ref, mag, U_BF16, c, extra))

    def grad(self, name, ref, mag, M, kind, extra=None):
        assert name not in self.expect, f"{name}: a second launch claims this gradient"
        self.expect[name] = (ref, mag, M, extra, kind)

    def bias_source(self, name, t, C, launch):
        """`name`.grad = the column sums of the stored tensor t; `launch`: a stand-alone colsum launch does it (else a fused pass)."""
        t2 = t[..., :C].double().reshape(-1, C)
        self.grad(name, t2.sum(0), t2.abs().sum(0), t2.shape[0], "param bias")
        if launch:
            self.want_colsums.append((self.own[name].grad.data_ptr(), t))

    def param(self, name, got, what):
        """The fp32 vector a launch was given must be the named parameter; -> its fp64 value."""
        p = self.own[name].data
        eq(got.reshape(-1)[:p.numel()], p.reshape(-1), f"{what}: {name}")
        return p.double().reshape(-1)

    def dest(self, c, arg, name, what):
        assert c.ptr.get(arg) == self.own[name].grad.data_ptr(), f"{what}: {arg} is not {name}.grad"

    # ---- stages
    def conv_fwd(self, mod, x, residual=None, what=""):
        c = self.it.next("conv_fwd")
        layer = self.mods[mod]
        assert c.mod == mod, (what, c.mod, mod)
        eq(c.a["x"], x, f"{what} {mod} input")
        if residual is None:
            assert c.a["residual"] is None, f"{what} {mod}: unexpected residual"
        else:
            eq(c.a["residual"], residual, f"{what} {mod} residual")
        assert c.a["act"] == 0 and c.a["scale"] is None and c.a["bias"] is None and not c.a["out_f32"]
        w = layer.kernel.data.double().reshape(layer.cin, layer.cout)
        b = layer.bias.data.double() if (layer.bias is not None and c.a["use_bias"]) else None
        assert (b is not None) == (oname(mod) + "/bias" in self.own), f"{what} {mod}: use_bias"
        ref, mag = R.dense(x[..., :layer.cin].double(), w, b, None if residual is None else residual[..., :layer.cout].double())
        self.b16("dense fwd", f"{what} {mod} y", c.out[..., :layer.cout], ref, mag)
        if layer.cout_p > layer.cout:
            assert c.out[..., layer.cout:].abs().max().item() == 0, "pad channels"
        return c.out

    def conv_bwd(self, mod, dy, x, skip_bias, what="", need_dx=True):
        c = self.it.next("conv_bwd")
        layer = self.mods[mod]
        pre = oname(mod)
        assert c.mod == mod, (what, c.mod, mod)
        eq(c.a["dy"], dy, f"{what} {mod} dy")
        eq(c.a["x"], x, f"{what} {mod} stored input")
        assert bool(c.a["skip_bias"]) == skip_bias, f"{what} {mod}: skip_bias is {c.a['skip_bias']}, the restatement says {skip_bias}"
        assert bool(c.a["need_dx"]) == need_dx and not c.a["skip_wgrad"] and c.a["dx_residual"] is None and not c.a["accumulate_dx"]
        w = layer.kernel.data.double().reshape(layer.cin, layer.cout)
        r = R.dense_bwd(x[..., :layer.cin].double(), w, dy[..., :layer.cout].double())
        M = dy[..., 0].numel()
        self.grad(pre + "/kernel", r["dw"], r["dwm"], M, "param kernel")
        if not skip_bias:
            self.bias_source(pre + "/bias", dy, layer.cout, launch=True)
        if not need_dx:
            assert c.out is None
            return None
        self.b16("dense dgrad", f"{what} {mod} dx", c.out[..., :layer.cin], r["dx"], r["dxm"])
        return c.out

    def ln_refs(self, x, dy, gam, bet):
        C = x.shape[-1]
        x2 = x.double().reshape(-1, C)
        d2 = None if dy is None else dy.double().reshape(-1, C)
        if C <= 512:
            r = norm_ref(x2, gam, bet, "none", dy=d2, eps=R.LN_EPS)
            r["yext"] = r["dgext"] = None
            return r
        return ln_wide_ref(x2, torch.zeros_like(x2) if d2 is None else d2, gam, bet)

    def ln_fwd(self, pre, x, what=""):
        C = x.shape[-1]
        wide = C > 512
        c = self.it.next("ln_wide_fwd" if wide else "norm_act_fwd")
        eq(c.a["x"], x, f"{what} {pre} input")
        assert abs(c.a["eps"] - R.LN_EPS) < 1e-12 and (wide or (c.a["mode"] == 0 and c.a["G"] == 1 and c.a["act"] == 0 and c.a["C_logical"] == C))
        gam, bet = self.param(pre + "/gamma", c.a["gamma"], what), self.param(pre + "/beta", c.a["beta"], what)
        r = self.ln_refs(x, None, gam, bet)
        self.b16("ln_wide fwd" if wide else "ln fwd", f"{what} {pre} y", c.out.reshape(-1, C), r["y"], r["ymag"], extra=r["yext"])
        return c.out

    def _ln_bwd_call(self, pre, x, dy, what, res=False):
        C = x.shape[-1]
        wide = C > 512
        c = self.it.next("norm_act_bwd_res" if res else ("ln_wide_bwd" if wide else "norm_act_bwd"))
        eq(c.a["x"], x, f"{what} {pre} stored input")
        eq(c.a["dy"], dy, f"{what} {pre} dy")
        assert abs(c.a["eps"] - R.LN_EPS) < 1e-12
        gam = self.param(pre + "/gamma", c.a["gamma"], what)
        bet = self.own[pre + "/beta"].data.double()
        self.dest(c, "dgamma", pre + "/gamma", what)
        self.dest(c, "dbeta", pre + "/beta", what)
        r = self.ln_refs(x, dy, gam, bet)
        M = x[..., 0].numel()
        self.grad(pre + "/gamma", r["dgamma"], r["dgmag"], M, "param ln", r["dgext"])
        self.grad(pre + "/beta", r["dbeta"], r["dbmag"], M, "param ln")
        return c, r, wide

    def ln_bwd(self, pre, x, dy, what=""):
        c, r, wide = self._ln_bwd_call(pre, x, dy, what)
        if not wide:
            assert c.a["dbias"] is None and c.a["mode"] == 0 and c.a["G"] == 1 and c.a["act"] == 0
        C = x.shape[-1]
        self.b16("ln_wide bwd" if wide else "ln bwd", f"{what} {pre} dx", c.out.reshape(-1, C), r["dx"], r["dxmag"])
        return c.out

    def ln_bwd_res(self, pre, x, dy, dres, dbias, what=""):
        """x + f(norm(x)) backward: -> the stored dx = LN'(dy) + dres; `dbias`: the bias whose gradient is the column sums of that dx."""
        C = x.shape[-1]
        assert C <= 512
        r64 = dres.double().reshape(-1, C)
        if self.run["fuse"]:
            c, r, _ = self._ln_bwd_call(pre, x, dy, what, res=True)
            eq(c.a["dres"], dres, f"{what} {pre} dres")
            # bf16(bf16(LN'(dy)) + dres): two roundings
            self.b16("ln bwd+res (fused)", f"{what} {pre} dx+res", c.out.reshape(-1, C), r["dx"] + r64, r["dxmag"] + r64.abs(), c=2 * C_BOUND)
            out = c.out
            if dbias is None:
                assert c.a["dbias"] is None, f"{what} {pre}: a dbias where the restatement has none"
            else:
                self.dest(c, "dbias", dbias, what)
                self.bias_source(dbias, out, C, launch=False)
            return out
        c, r, _ = self._ln_bwd_call(pre, x, dy, what)
        assert c.a["dbias"] is None
        dx1 = c.out
        self.b16("ln bwd", f"{what} {pre} dx", dx1.reshape(-1, C), r["dx"], r["dxmag"])
        c2 = self.it.next("copy_channels")
        assert c2.a["accumulate"]
        eq(c2.a["src"], dres, f"{what} {pre} accumulate source")
        eq(c2.a["dst"], dx1, f"{what} {pre} accumulate destination")
        out = c2.post["dst"]
        d64 = dx1.double().reshape(-1, C)
        self.b16("copy+=", f"{what} {pre} +res", out.reshape(-1, C), d64 + r64, d64.abs() + r64.abs())
        # the two launches as one stage: LN'(dy) rounded to bf16, then the sum rounded again - the second rounding doubles the constant
        self.b16("ln bwd+res (unfused)", f"{what} {pre} dx+res", out.reshape(-1, C), r["dx"] + r64, r["dxmag"] + r64.abs(), c=2 * C_BOUND)
        if dbias is not None:
            self.bias_source(dbias, out, C, launch=True)
        return out

    # ---- the model
    def forward(self):
        run, net, it = self.run, self.net, self.it
        cfg = R.CFG
        c = it.next("patchify")
        assert c.a["patch"] == cfg["patch_size"]
        eq(c.a["x"], run["x"], "patchify input")
        eq(c.out, R.patchify(run["x"].double(), cfg["patch_size"]).to(BF16), "patchify")
        self.emb_p = c.out
        self.emb_t = self.conv_fwd("patch_embed.proj", c.out, what="embed")
        t = self.ln_fwd("patch_embed/norm", self.emb_t, "embed")
        if run["variant"] == "ape":
            src = self.own["absolute_pos_embed"].data.to(BF16).reshape(1, *R.stage_res(0), cfg["embed_dim"])
            parts = []
            for b in range(R.BATCH):
                c = it.next("copy_channels")
                assert c.a["accumulate"]
                eq(c.a["src"], src, "ape source")
                eq(c.a["dst"], t[b:b + 1], "ape destination")
                s64, d64 = src.double(), t[b:b + 1].double()
                self.b16("copy+=", f"ape image {b}", c.post["dst"], s64 + d64, s64.abs() + d64.abs())
                parts.append(c.post["dst"])
            t = torch.cat(parts)
        ns = len(cfg["depths"])
        self.stage_out, self.merge_fw = {}, {}
        for s in range(ns):
            for i in range(cfg["depths"][s]):
                t = self.block_fwd(s, i, t)
            if s < ns - 1:
                self.stage_out[s] = t
                eq(run["feats"][s].reshape(t.shape), t, f"feature {s}")
                c = it.next("patch_merge")
                assert not c.a["backward"]
                eq(c.a["full"], t, f"merge {s} input")
                m = c.post["merged"]
                eq(m, R.patch_merge(t), f"merge {s}")
                n = self.ln_fwd(f"layers{s}/downsample/norm", m, f"merge {s}")
                self.merge_fw[s] = (m, n)
                t = self.conv_fwd(f"basic_layers.{s}.downsample.reduction", n, what=f"merge {s}")
        self.last_in = t
        self.last = self.ln_fwd("norm", t, "tail")
        c = it.next("token_mean_fwd")
        eq(c.a["x"], self.last, "token mean input")
        m, mm = R.token_mean(self.last.double())
        L = self.last.shape[1] * self.last.shape[2]
        self.note("token_mean", acheck(f"{self.tag} token mean", c.out, m, mm, U_F32, c_f32(L)))
        self.pooled = c.out
        if run["variant"] == "top":
            self.pooled_bf = c.out.to(BF16).reshape(R.BATCH, 1, 1, -1)
            y = self.conv_fwd("head", self.pooled_bf, what="head")
            c = it.next("to_f32")
            eq(c.a["x"], y, "logits cast input")
            eq(c.out, y[..., :R.NUM_CLASSES].float(), "logits cast")
            eq(run["out"], c.out.reshape(R.BATCH, R.NUM_CLASSES), "model output")
        else:
            eq(run["out"], c.out, "model output")

    def block_fwd(self, s, i, x):
        it, cfg = self.it, R.CFG
        pre, mod, what = f"layers{s}/blocks{i}/", f"basic_layers.{s}.blocks.{i}.", f"stage {s} block {i}"
        f = {"x": x}
        f["n1"] = self.ln_fwd(pre + "norm1", x, what)
        f["qkv"] = self.conv_fwd(mod + "attn.qkv", f["n1"], what=what)
        c = it.next("window_attn_fwd")
        wsz, shift = S.block_window(R.stage_res(s), cfg["window_size"], i)
        eq(c.a["qkv"], f["qkv"], f"{what} window input")
        assert (c.a["heads"], c.a["ws"], c.a["shift"]) == (cfg["num_heads"][s], wsz, shift), (what, c.a["heads"], c.a["ws"], c.a["shift"])
        self.param(pre + "attn/relative_position_bias_table", c.a["table"], what)
        f["ctx"] = c.out                    # bounded in block_bwd, where window_ref runs once for both directions
        f["a"] = self.conv_fwd(mod + "attn.proj", f["ctx"], residual=x, what=what)
        f["n2"] = self.ln_fwd(pre + "norm2", f["a"], what)
        f["h"] = self.conv_fwd(mod + "mlp.fc1", f["n2"], what=what)
        c = it.next("act_fwd")
        from ultrasound_modeling_amd.ops import ACT_GELU
        eq(c.a["x"], f["h"], f"{what} GELU input")
        assert c.a["act"] == ACT_GELU
        g64 = R.gelu(f["h"].double())
        self.b16("gelu", f"{what} gelu", c.out, g64, g64.abs())
        f["g"] = c.out
        f["y"] = self.conv_fwd(mod + "mlp.fc2", f["g"], residual=f["a"], what=what)
        self.fw[s, i] = f
        return f["y"]

    def block_bwd(self, s, i, dy, done, prev):
        """`done`: the launch that produced dy also summed it into this block's fc2.bias.grad; `prev`: the fc2 bias of the block below,
        whose gradient is the column sums of this block's dx."""
        from ultrasound_modeling_amd.ops import ACT_GELU
        it, cfg, f = self.it, R.CFG, self.fw[s, i]
        pre, mod, what = f"layers{s}/blocks{i}/", f"basic_layers.{s}.blocks.{i}.", f"stage {s} block {i}"
        skip = R.skip_bias(done)
        dg = self.conv_bwd(mod + "mlp.fc2", dy, f["g"], skip["mlp/fc2"], what)
        c = it.next("act_bwd_colsum")
        eq(c.a["x"], f["h"], f"{what} GELU backward pre-activation")
        eq(c.a["dy"], dg, f"{what} GELU backward dy")
        assert c.a["act"] == ACT_GELU and c.a["C_logical"] == f["h"].shape[-1]
        self.dest(c, "db", pre + "mlp/fc1/bias", what)
        dh64 = R.gelu_d(f["h"].double()) * dg.double()
        self.b16("gelu bwd", f"{what} dh", c.out, dh64, dh64.abs())
        dh = c.out
        self.bias_source(pre + "mlp/fc1/bias", dh, dh.shape[-1], launch=False)
        dn2 = self.conv_bwd(mod + "mlp.fc1", dh, f["n2"], skip["mlp/fc1"], what)
        da = self.ln_bwd_res(pre + "norm2", f["a"], dn2, dy, pre + "attn/proj/bias", what)
        dctx = self.conv_bwd(mod + "attn.proj", da, f["ctx"], skip["attn/proj"], what)
        c = it.next("window_attn_bwd")
        wsz, shift = S.block_window(R.stage_res(s), cfg["window_size"], i)
        heads = cfg["num_heads"][s]
        eq(c.a["qkv"], f["qkv"], f"{what} window backward qkv")
        eq(c.a["dout"], dctx, f"{what} window backward dout")
        assert (c.a["heads"], c.a["ws"], c.a["shift"]) == (heads, wsz, shift)
        table = self.param(pre + "attn/relative_position_bias_table", c.a["table"], what).reshape(-1, heads)
        self.dest(c, "dtable", pre + "attn/relative_position_bias_table", what)
        r = window_ref(f["qkv"].double(), dctx.double(), table, heads, wsz, shift, list(range(R.BATCH)))
        kind = "window mfma" if (wsz == 8 and f["x"].shape[-1] // heads == 32) else "window generic"
        self.b16(kind + " fwd", f"{what} ctx", f["ctx"], r["o"], r["om"], extra=r["oext"])
        self.b16(kind + " bwd", f"{what} dqkv", c.out, r["dqkv"], r["dqkvm"], extra=r["dqkvext"])
        self.grad(pre + "attn/relative_position_bias_table", r["dtable"], r["dtablem"], f["x"][..., 0].numel(), "param table", r["dtableext"])
        dqkv = c.out
        dn1 = self.conv_bwd(mod + "attn.qkv", dqkv, f["n1"], skip["attn/qkv"], what)
        return self.ln_bwd_res(pre + "norm1", f["x"], dn1, da, prev, what)

    def backward(self):
        run, it, cfg = self.run, self.it, R.CFG
        ns = len(cfg["depths"])
        if run["variant"] == "top":
            dy = torch.zeros(R.BATCH, 1, 1, 16, dtype=BF16, device=DEV)
            dy[..., :R.NUM_CLASSES] = run["d_out"].reshape(R.BATCH, 1, 1, -1).to(BF16)
            dx = self.conv_bwd("head", dy, self.pooled_bf, False, "head")
            c = it.next("to_f32")
            eq(c.a["x"], dx, "head dx cast input")
            eq(c.out, dx.float(), "head dx cast")
            dpool = c.out.reshape(R.BATCH, -1)
        else:
            dpool = run["d_out"]
        c = it.next("token_mean_bwd")
        eq(c.a["dy"], dpool, "token mean backward dy")
        eq(c.a["like"], self.last, "token mean backward shape donor")
        want = R.token_mean_bwd(dpool.double(), self.last)
        self.b16("token_mean bwd", "token mean dx", c.out, want, want.abs())
        d = self.ln_bwd("norm", self.last_in, c.out, "tail")
        for s in reversed(range(ns)):
            if s < ns - 1:
                m, n = self.merge_fw[s]
                dn = self.conv_bwd(f"basic_layers.{s}.downsample.reduction", d, n, True, f"merge {s}")
                dm = self.ln_bwd(f"layers{s}/downsample/norm", m, dn, f"merge {s}")
                c = it.next("patch_merge")
                assert c.a["backward"]
                eq(c.a["merged"], dm, f"merge {s} backward input")
                dx = c.post["full"]
                eq(dx, R.patch_unmerge(dm), f"merge {s} backward")
                c = it.next("copy_channels")
                assert c.a["accumulate"]
                df = run["dfs"][s].reshape(dx.shape)
                eq(c.a["src"], df, f"stage {s}: the accumulated tensor is not d_features[{s}]")
                eq(c.a["dst"], dx, f"stage {s}: d_features[{s}] is not added to downsample.backward(...)")
                self.b16("copy+=", f"stage {s} + d_feature", c.post["dst"], dx.double() + df.double(), dx.double().abs() + df.double().abs())
                d = c.post["dst"]
            depth = cfg["depths"][s]
            done = False
            for i in reversed(range(depth)):
                prev = f"layers{s}/blocks{i - 1}/mlp/fc2/bias" if i > 0 else None
                d = self.block_bwd(s, i, d, done, prev)
                done = prev is not None
        if run["variant"] == "ape":
            c = it.next("to_f32")
            eq(c.a["x"], d, "ape gradient cast input")
            eq(c.out, d.float(), "ape gradient cast")
            self.grad("absolute_pos_embed", d.double().sum(0).reshape(-1), d.double().abs().sum(0).reshape(-1), R.BATCH, "param ape")
        d = self.ln_bwd("patch_embed/norm", self.emb_t, d, "embed")
        self.conv_bwd("patch_embed.proj", d, self.emb_p, False, "embed", need_dx=False)
        it.done()

    def gradients(self):
        """Every parameter gradient exactly once, and every stand-alone colsum launch accounted for."""
        assert set(self.expect) == set(self.own), (set(self.own) - set(self.expect), set(self.expect) - set(self.own))
        for name, (ref, mag, M, extra, kind) in self.expect.items():
            g = self.own[name].grad
            self.note(kind, acheck(f"{self.tag} {name}.grad", g.reshape(-1), ref.reshape(-1), mag.reshape(-1), U_F32, c_f32(M),
                                   None if extra is None else extra.reshape(-1)))
        left = list(self.want_colsums)
        for c in self.colsums:
            hit = [k for k, (ptr, t) in enumerate(left) if ptr == c.ptr["db"] and t.shape == c.a["dy"].shape and torch.equal(t, c.a["dy"])]
            assert hit, "a colsum launch the restatement does not have (wrong destination or wrong tensor)"
            left.pop(hit[0])
        assert not left, f"{len(left)} bias sums the restatement has were never launched"

    def kernels(self):
        """Every route of the configuration was reached, and its first launch showed the kernels named for it (asserted by routed when it
        ran); the deferred sums of the backward pass finish at the end of the overlap region, probed there."""
        missing = set(self.run["routes"]) - set(self.run["seen"])
        assert not missing, f"routes the configuration should reach but did not: {sorted(missing, key=str)}"


def stage_checks(run):
    w = Walk(run)
    w.forward()
    w.backward()
    w.gradients()
    w.kernels()


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "inline"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_stage_checks(monkeypatch, fuse, lazy):
    stage_checks(get_run(monkeypatch, "plain", fuse, lazy))


@pytest.mark.parametrize("variant", ["ape", "top"])
def test_stage_checks_variants(monkeypatch, variant):
    stage_checks(get_run(monkeypatch, variant, True, True))


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_lazy_block_gradients_bit_identical(monkeypatch, fuse):
    a, b = get_run(monkeypatch, "plain", fuse, True), get_run(monkeypatch, "plain", fuse, False)
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["grad"], b["grad"]), f"{(a['grad'] != b['grad']).sum().item()} gradient entries differ between _LAZY_BLOCK 1 and 0"
    assert a["grad"].abs().sum().item() > 0


def oracle(variant):
    if variant not in _ORACLE:
        P = R.make_params(variant)
        x, d_out, dfs = R.make_inputs(variant)
        leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        out, feats = S.swin_forward(x, leaves, R.cfg_of(variant))
        grads = torch.autograd.grad([out] + feats, list(leaves.values()), [d_out] + dfs)
        _ORACLE[variant] = (out.detach(), [f.detach() for f in feats], dict(zip(leaves, grads)))
    return _ORACLE[variant]


@pytest.mark.parametrize("variant,fuse,lazy", [("plain", True, True), ("plain", False, False), ("top", True, True), ("ape", True, True)],
                         ids=["plain", "plain_unfused_inline", "top", "ape"])
def test_model_against_the_oracle_with_d_features(monkeypatch, variant, fuse, lazy):
    """The relative-L2 bars of test_small_swin_model_against_the_oracle, unchanged, with the stage outputs differentiated."""
    run = get_run(monkeypatch, variant, fuse, lazy)
    want, feats_r, grads = oracle(variant)
    e_o = rel(run["out"], want)
    e_f = [rel(f, fr) for f, fr in zip(run["feats"], feats_r)]
    errs = sorted((rel(p.grad.reshape(grads[k].shape), grads[k]), k) for k, p in run["own"].items())
    print(f"\n  {run['tag']}: out rel {e_o:.3e} feature rel {e_f} grad median {errs[len(errs) // 2][0]:.3e} worst {errs[-1]}", end="")
    assert len(e_f) == 2 and e_o < 2e-2 and max(e_f) < 2e-2
    assert errs[len(errs) // 2][0] < 3e-2 and errs[-1][0] < 1.5e-1
    if variant == "top":
        assert {"head/kernel", "head/bias"} <= {k for _, k in errs}


def test_zz_worst_ratio_table(monkeypatch):
    """Prints the worst err / bound per stage kind and switch combination of the runs above (run alone: of the default switches)."""
    if not WORST:
        stage_checks(get_run(monkeypatch, "plain", True, True))
    tags = sorted({t for t, _ in WORST})
    for kind in sorted({k for _, k in WORST}):
        print(f"\n  worst ratio {kind:22s} " + "  ".join(f"[{t}] {WORST[t, kind]:.3f}" for t in tags if (t, kind) in WORST), end="")
    assert max(WORST.values()) <= 1.0
