"""tools/timing.py on the device: the number of times a timed callable runs, that the step windows add no hidden optimisation steps, and
one converted script (tools/time_topk.py) end to end at a toy shape."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timing  # noqa: E402


def _finite_positive(ts, n):
    return len(ts) == n and all(math.isfinite(t) and t > 0 for t in ts)


def test_time_calls_runs_each_callable_as_often_as_its_docstring_says():
    from ultrasound_modeling_amd import ops
    ca, cb = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    ts = timing.time_calls({"a": lambda: ops.counter_add(ca, 1), "b": lambda: ops.counter_add(cb, 1)}, rounds=2, reps=3, replays=2, warm=2)
    torch.cuda.synchronize()
    assert "warm + reps * (1 + rounds * replays)" in timing.time_calls.__doc__
    assert ca.item() == cb.item() == 2 + 3 * (1 + 2 * 2) == 17                   # warm-up, the capture (no run), the untimed replay, the windows
    assert list(ts) == ["a", "b"] and _finite_positive(ts["a"], 2) and _finite_positive(ts["b"], 2), ts


def test_time_steps_adds_no_hidden_steps():
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    kw = dict(batch_size=2, img_size=(64, 64), in_channels=1)
    x, y = timing.bleed_batch(2, 64, 64, 1, torch.Generator().manual_seed(0))
    assert x.shape == (2, 64, 64, 1) and y.shape == (2, 64, 64, 3) and sorted(y.argmax(-1).unique().tolist()) == [0, 1, 2]
    timed, plain = VisionTransformer(**kw), VisionTransformer(**kw)
    assert torch.equal(timed.flat.flat, plain.flat.flat)
    timed.capture_graph(x, y)
    ts = timing.time_steps(lambda: timed.train_step(x, y), rounds=2, replays=2, warm=1)
    assert _finite_positive(ts, 2), ts
    for _ in range(1 + 2 * 2):
        plain.train_step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(timed.flat.flat, plain.flat.flat)


def test_time_topk_end_to_end_at_a_toy_shape(tmp_path):
    """2 x 64 x 64 is the smallest shape the existing step tests build; every size the script derives (H/2, W/2, H/3, H/8) is non-zero there."""
    out = tmp_path / "topk.json"
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join("tools", "time_topk.py"), "--loss", "cce", "--rounds", "1", "--replays", "1", "--reps", "1",
           "--json", str(out), "2", "64", "64"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    got = json.load(open(out))
    want = json.load(open(os.path.join(ROOT, "profiles", "topk_step.json")))
    assert set(got) == {"shape", "launch_us", "step_ms"} and got["shape"] == [2, 64, 64]
    row_keys = set(next(iter(want["launch_us"].values())))
    assert set(got["launch_us"]) == set(want["launch_us"])
    for name, row in got["launch_us"].items():
        assert set(row) == row_keys, name
        assert math.isfinite(row["median"]) and row["min"] <= row["median"] <= row["max"] and row["min"] > 0, (name, row)
    step = got["step_ms"]["this:cce"]
    assert set(step) == {"min", "median", "max", "rounds", "vs_cce_us"} and len(step["rounds"]) == 1 and step["median"] > 0
