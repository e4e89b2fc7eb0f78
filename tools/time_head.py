"""Times the fused head launch (head conv + softmax + loss + d loss / d logits, csrc/attn_loss_optim.hip head_quad_loss_kernel) at the bench
shape with tools/time_conv.py's method: `reps` launches captured into one HIP graph, replayed three times between two events.
usage: python tools/time_head.py [--lib PATH] [--rounds N] [B h w Cin C]
  --lib PATH: time that build of the library instead (e.g. the parent commit's, which has only the CategoricalCrossentropy entry point);
  each variant is timed `rounds` times, the variants alternating inside every round (tools/timing.py), so the spread stands beside every number.
With a library that has the region-overlap losses (csrc/overlap_loss.hip) it also times, in the same process, the path they take - the
probabilities-only head launch, the sums pass and the backward pass, together and one by one - and the softmax_loss kernel on the same
pixels, and prints each kernel's achieved bytes/s against the bytes it must move."""
import argparse
import ctypes as C
import sys

import torch

import timing

sys.path.insert(0, ".")
from ultrasound_modeling_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=L.LIB_PATH)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("shape", nargs="*", type=int, default=[16, 128, 128, 72, 3])
a = ap.parse_args()
B, h, w, Cin, NC = a.shape
lib = C.CDLL(a.lib)
L.bind(lib, ["usseg_head_quad_softmax_loss"])
has_cl = hasattr(lib, "usseg_head_quad_softmax_loss_cl")
if has_cl:
    L.bind(lib, ["usseg_head_quad_softmax_loss_cl"])

g = torch.Generator().manual_seed(0)
x = torch.randn(B, h, w, Cin, generator=g).to(torch.bfloat16).cuda()
wq = (torch.randn(16, 9 * Cin, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16).cuda()
bias = torch.zeros(4).cuda()
y = torch.softmax(torch.randn(B, 2 * h, 2 * w, NC, generator=g), -1).cuda()
probs = torch.empty(B, 2 * h, 2 * w, NC).cuda()
loss = torch.zeros(L.ACC_FLOATS).cuda()
dl = torch.empty(B, h, w, 16, dtype=torch.bfloat16).cuda()


def launch(cl):
    s = torch.cuda.current_stream().cuda_stream
    args = [x.data_ptr(), B, h, w, Cin, Cin, wq.data_ptr(), bias.data_ptr(), NC, y.data_ptr(), probs.data_ptr(), loss.data_ptr(), dl.data_ptr(), 0.1, 1e-7,
            1.0 / B]
    rc = lib.usseg_head_quad_softmax_loss(*args, s) if cl is None else lib.usseg_head_quad_softmax_loss_cl(*args, C.byref(cl), s)
    assert rc == 0, rc


variants = [("cce (loss_kind 0)", None)]
if has_cl:
    cf = (C.c_float * 8)(0.06329, 0.027567, 0.90914)
    variants += [("my_loss_cat (gamma 0)", L.ClassLoss(cf, 0.0, 3.0)), ("focal (gamma 2)", L.ClassLoss((C.c_float * 8)(*([1.0] * 8)), 2.0, 1.0))]
print(f"{a.lib}: fused head {B}x{h}x{w} {Cin} channels, {NC} classes")
timing.require_gpu("time_head")
for name, ts in timing.time_calls({name: lambda cl=cl: launch(cl) for name, cl in variants}, a.rounds, a.reps, replays=3).items():
    s = timing.spread(ts, 2)
    print(f"  {name:24s} {s['min']:7.2f} us min, {s['median']:7.2f} median, {s['max']:7.2f} max   [{' '.join(f'{v:.2f}' for v in ts)}]")

if hasattr(lib, "usseg_overlap_loss_sums"):
    L.bind(lib, ["usseg_overlap_loss_sums", "usseg_overlap_loss_bwd", "usseg_softmax_loss_fwd_bwd"])
    H, W = 2 * h, 2 * w
    M = B * H * W
    from ultrasound_modeling_amd import ops
    acc = torch.zeros(ops.OVERLAP_ACC_FLOATS).cuda()
    logits = torch.randn(B, h, w, 16, generator=g).cuda()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    dq = L.LossDesc(M, H * W, NC, 16, 16, 0, 0.1, 1e-7, 1.0 / B, W)

    def head_probs_only():
        rc = lib.usseg_head_quad_softmax_loss(x.data_ptr(), B, h, w, Cin, Cin, wq.data_ptr(), bias.data_ptr(), NC, None, probs.data_ptr(), None, None, 0.1, 1e-7,
                                              1.0 / B, stream())
        assert rc == 0, rc

    def sums(ol):
        assert lib.usseg_overlap_loss_sums(C.byref(dq), C.byref(ol), 1.0, probs.data_ptr(), y.data_ptr(), acc.data_ptr(), acc.numel(), stream()) == 0

    def bwd(ol):
        assert lib.usseg_overlap_loss_bwd(C.byref(dq), C.byref(ol), probs.data_ptr(), y.data_ptr(), acc.data_ptr(), acc.numel(), dl.data_ptr(), stream()) == 0

    def softmax_loss():
        assert lib.usseg_softmax_loss_fwd_bwd(C.byref(dq), logits.data_ptr(), y.data_ptr(), None, probs.data_ptr(), loss.data_ptr(), dl.data_ptr(), stream()) == 0

    uw = (C.c_float * 8)(*([1.0 / NC] * NC))
    rd = 2 * M * NC * 4
    named = {"head, probabilities only": (head_probs_only, None)}                 # name -> (fn, bytes it must move)
    for name, ol in (("dice", L.OverlapLoss(uw, 0.5, 0.5, 1.0, 1.0, 1.0, 0.0)), ("dice_ce", L.OverlapLoss(uw, 0.5, 0.5, 1.0, 1.0, 1.0, 1.0))):
        named[f"{name}: head + sums + bwd"] = (lambda ol=ol: (head_probs_only(), sums(ol), bwd(ol)), None)
        named[f"{name}: sums (pass 1)"] = (lambda ol=ol: sums(ol), rd)
        named[f"{name}: bwd (pass 2)"] = (lambda ol=ol: bwd(ol), rd + M * 8)
    # softmax_loss_kernel: quad fp32 logits read (64 B per 2x2 pixels = 16 B a pixel), labels read AND probabilities written (2 * M*NC*4), dlogits written (8 B a pixel)
    named["softmax_loss (quad logits, cce)"] = (softmax_loss, M * 16 + 2 * M * NC * 4 + M * 8)
    ts = timing.time_calls({n: fn for n, (fn, _) in named.items()}, a.rounds, a.reps, replays=3)
    for name, (_, nbytes) in named.items():
        s = timing.spread(ts[name], 2)
        bw = "" if nbytes is None else f"   {nbytes / 1e6:6.1f} MB -> {nbytes / s['median'] / 1e6:5.2f} TB/s"
        print(f"  {name:40s} {s['min']:7.2f} us min, {s['median']:7.2f} median, {s['max']:7.2f} max{bw}")
