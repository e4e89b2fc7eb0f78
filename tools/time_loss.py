import sys, torch
import timing
sys.path.insert(0, ".")
from ultrasound_modeling_amd import ops
B, H, W, C = 16, 256, 256, 3
logits = torch.randn(B, H // 2, W // 2, 16, device="cuda")
y = torch.softmax(torch.randn(B, H, W, C, device="cuda"), -1)
probs = torch.empty(B, H, W, C, device="cuda")
loss = torch.zeros(ops.ACC_FLOATS, device="cuda")
dl = torch.empty(B, H // 2, W // 2, 16, dtype=torch.bfloat16, device="cuda")
big = torch.empty(256 * 1024 * 1024 // 4, device="cuda")
def run(): ops.softmax_loss(logits, y, probs, loss, dl, HW=H * W, C_classes=C, loss_kind=0, inv_global_batch=1 / 16, quad_w=W)
# (one event pair per call with the cache flushed OUTSIDE the pair: the one protocol here that tools/timing.py does not offer)
for _ in range(3): run()
for flush in (False, True):
    ts = []
    for _ in range(10):
        if flush: big.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    print("flush" if flush else "hot", [f"{t:.1f}" for t in ts])

# ---- the boundary term: sdf_labels alone, then the two passes of the overlap + boundary pair ---------------------
def _time(fn, n=10):
    sp = timing.spread([ms * 1e3 for ms in timing.time_steps(fn, n, 1, warm=3)])         # eager, one call a window
    return sp["median"], sp["min"], sp["max"]

g = torch.Generator().manual_seed(0)
lab = torch.rand(B, H // 16, W // 16, generator=g)                      # bench.py's labels: 16x16 blocks, about 30 % class 1/2
lab = ((lab > 0.70).float() + (lab > 0.95).float()).repeat_interleave(16, 1).repeat_interleave(16, 2)
blocks = torch.nn.functional.one_hot(lab.long(), C).float().cuda().contiguous()
yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
blob = ((yy - 40) ** 2 + (xx - 200) ** 2 <= 12 ** 2).float()            # one small bleed per image: the far pixels scan the longest columns
blobs = torch.stack([1 - blob, torch.zeros_like(blob), blob], -1).expand(B, H, W, C).contiguous().cuda()
acc = torch.zeros(ops.OVERLAP_ACC_FLOATS, device="cuda")
wb = torch.tensor([0.01], device="cuda")
ol, bl = ops.overlap_loss([1 / 3] * 3), ops.boundary_loss([0.0, 1.0, 1.0])
kw = dict(overlap=ol, HW=H * W, C_classes=C, inv_global_batch=1 / 16)
for name, yl in (("blocks", blocks), ("one blob", blobs)):
    phi = torch.empty_like(yl)
    ws = torch.empty(ops.sdf_ws_bytes(B, H, W, C), dtype=torch.uint8, device="cuda")
    print(f"{name}: sdf_labels {B}x{H}x{W}x{C} us (median, min, max)", ["%.1f" % t for t in _time(lambda: ops.sdf_labels(yl, phi, ws))],
          "max |phi| %.1f" % phi.abs().max().item())
    print(f"{name}: overlap_loss_sums", ["%.1f" % t for t in _time(lambda: ops.overlap_loss_sums(probs, yl, acc, **kw))],
          "+ boundary", ["%.1f" % t for t in _time(lambda: ops.overlap_boundary_loss_sums(probs, yl, phi, acc, boundary=bl, wb=wb, **kw))])
    print(f"{name}: overlap_loss_bwd", ["%.1f" % t for t in _time(lambda: ops.overlap_loss_bwd(probs, yl, acc, dl, quad_w=W, **kw))],
          "+ boundary", ["%.1f" % t for t in _time(lambda: ops.overlap_boundary_loss_bwd(probs, yl, phi, acc, dl, boundary=bl, quad_w=W, **kw))])
