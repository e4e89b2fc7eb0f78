"""tools/timing.py without a device: the statistics, the order of the windows, the refusal to time on the host, the child protocol of
``alternate_trees`` (driven with a plain-Python child that needs neither torch nor a GPU), and that every converted script still parses
its command line."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import timing  # noqa: E402

# the converted scripts: those that parse with argparse, and those that read sys.argv by hand (or take no arguments and start at once)
ARGPARSE = ["time_average", "time_cascade", "time_cone", "time_distill", "time_ensemble", "time_head", "time_lovasz", "time_optim", "time_predict",
            "time_prepaug", "time_scores", "time_surface", "time_sweep", "time_topk", "time_warp"]
BY_HAND = ["bench_conv", "bench_fused_dgrad", "bench_launch", "bench_norm", "exp_streams", "time_cardinal", "time_components", "time_conv", "time_flash",
           "time_gemm", "time_loss"]


def test_spread_takes_the_upper_median():
    assert timing.spread([3.0, 1.0, 2.0], 4) == {"min": 1.0, "median": 2.0, "max": 3.0}
    assert timing.spread([4.0, 1.0, 3.0, 2.0], 4) == {"min": 1.0, "median": 3.0, "max": 4.0}          # even: the upper of the two middle ones
    assert timing.spread([5.0], 4) == {"min": 5.0, "median": 5.0, "max": 5.0}
    assert timing.spread([1.23456, 1.23444], 2) == {"min": 1.23, "median": 1.23, "max": 1.23}
    assert timing.spread([0.5, 0.25])["median"] == 0.5


def test_schedule_is_round_major():
    assert timing.schedule(["a", "b", "c"], 2) == [(0, "a"), (0, "b"), (0, "c"), (1, "a"), (1, "b"), (1, "c")]
    assert timing.schedule(["a"], 0) == []


def test_nothing_is_timed_without_a_device(monkeypatch):
    monkeypatch.setattr(timing.torch.cuda, "is_available", lambda: False)
    calls = []
    with pytest.raises(SystemExit) as e:
        timing.require_gpu("some_script")
    assert "some_script" in str(e.value.code) and "GPU" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        timing.time_calls({"a": lambda: calls.append(1)}, rounds=2, reps=3, replays=2)
    assert e.value.code not in (0, None)
    with pytest.raises(SystemExit):
        timing.time_steps(lambda: calls.append(1), rounds=2, replays=2)
    assert calls == []


CHILD = """import json, os, sys, time
assert sys.argv[1] == "--child"
root, label, log, mode = sys.argv[2:6]
with open(log, "a") as f:
    f.write(label + "\\n")
n = len(open(log).read().split())
if mode == "fail" and n == 3:
    print("about to fail", flush=True)
    sys.exit(3)
if mode == "hang" and n == 3:
    time.sleep(30)
print("noise")
print("TAG " + json.dumps({"stale": -1}))
print("TAG " + json.dumps({"root": root, "n": n}), flush=True)
print("TAGGED but not the tag")
"""


def _drive(tmp_path, mode, timeout=60):
    script, log = tmp_path / "child.py", tmp_path / "log.txt"
    script.write_text(CHILD)
    trees = [("this", "/here", ["this"]), ("parent", "/there", ["parent"])]
    try:
        return timing.alternate_trees(str(script), trees, 2, "TAG", [str(log), mode], timeout), log.read_text().split()
    except SystemExit as e:
        return e, log.read_text().split()


def test_alternate_trees_alternates_fresh_children(tmp_path):
    runs, log = _drive(tmp_path, "ok")
    assert log == ["this", "parent", "this", "parent"]
    assert runs == {"this:root": ["/here", "/here"], "this:n": [1, 3], "parent:root": ["/there", "/there"], "parent:n": [2, 4]}


@pytest.mark.parametrize("mode,status", [("fail", "exit 3"), ("hang", "killed after 1 s")])
def test_alternate_trees_starts_nothing_after_a_failure(tmp_path, mode, status):
    e, log = _drive(tmp_path, mode, timeout=60 if mode == "fail" else 1)
    assert isinstance(e, SystemExit), e
    msg = str(e.code)
    assert "this tree" in msg and "round 1" in msg and status in msg, msg
    if mode == "fail":
        assert "about to fail" in msg                                                       # the tail of the child's stdout
    assert log == ["this", "parent", "this"]                                                 # the third child failed: there was no fourth


def test_timing_imports_without_the_package():
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    code = "import sys, timing; assert not any(m.split('.')[0] == 'ultrasound_modeling_amd' for m in sys.modules); print('ok')"
    p = subprocess.run([sys.executable, "-c", code], cwd=TOOLS, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


def test_every_timing_script_is_accounted_for():
    """The scripts that hold a timing primitive of their own are the module and the two left alone on purpose: launch_table.py brackets every
    call site of ONE eager step, time_loss.py's first table flushes the cache between calls outside the event pair."""
    own = [f[:-3] for f in sorted(os.listdir(TOOLS)) if f.endswith(".py")
           and any(k in open(os.path.join(TOOLS, f)).read() for k in ("CUDAGraph()", "enable_timing=True"))]
    assert own == ["launch_table", "time_loss", "timing"]
    for name in ARGPARSE + BY_HAND:
        src = open(os.path.join(TOOLS, name + ".py")).read()
        assert "import timing" in src and ("argparse" in src) == (name in ARGPARSE), name


@pytest.mark.parametrize("name", ARGPARSE)
def test_converted_script_parses_its_command_line(name):
    p = subprocess.run([sys.executable, os.path.join("tools", name + ".py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and "usage" in p.stdout.lower(), (p.stdout[-1000:], p.stderr[-2000:])
