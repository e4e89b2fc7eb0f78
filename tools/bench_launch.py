import sys, torch
import timing
sys.path.insert(0, ".")
from ultrasound_modeling_amd import ops
timing.require_gpu("bench_launch")
dev = torch.device("cuda:0")
x = torch.zeros(16, device=dev)
big = torch.zeros(64 << 20, device=dev)   # 256 MB
def timeit(fn, reps):
    """`reps` launches in one HIP graph, one window of ten replays between two device events: seconds per launch."""
    return timing.window_us(timing.graph_of(fn, reps), reps, 10) * 1e-6
print("trivial fill (1 WG):        %.2f us per launch" % (timeit(lambda: ops.fill_f32(x, 0.0), 200) * 1e6))
y = torch.zeros(1 << 20, device=dev)
print("fill 4 MB:                  %.2f us per launch" % (timeit(lambda: ops.fill_f32(y, 0.0), 200) * 1e6))
print("torch zero_ 64 B:           %.2f us per launch" % (timeit(lambda: x.zero_(), 200) * 1e6))
