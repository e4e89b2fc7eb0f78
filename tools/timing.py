"""The one timing protocol of the scripts under tools/ (DESIGN.md section 5).

A call is warmed up, `reps` of it are captured into one HIP graph, and a window is `replays` replays of that graph between two device
events: microseconds per call = elapsed / (replays * reps).  Calls that are compared are timed in the same process, alternating inside
every round (``schedule``), and a figure is the min / upper median / max over the rounds (``spread``).  A step that is already a graph
(``capture_graph``) is timed by ``time_steps``; two checkouts are compared by ``alternate_trees``, one fresh process per tree and round.

This module never imports the package at module level: it is always loaded from THIS tree, next to the script that uses it, while the
package may come from another checkout (``alternate_trees``)."""
import json
import os
import subprocess
import sys

import torch


def require_gpu(who):
    """Exit unless there is a device: a timing on the host says nothing, so nothing falls back to one."""
    if not torch.cuda.is_available():
        sys.exit(f"{who}: needs a GPU (a timing on the host says nothing)")


def spread(ts, digits=4):
    """{"min", "median", "max"} of ts, rounded.  The median is the UPPER one, sorted(ts)[len(ts) // 2]: the form the committed
    profiles/*.json were made with, so that old and new files stay comparable."""
    ts = sorted(ts)
    return {"min": round(ts[0], digits), "median": round(ts[len(ts) // 2], digits), "max": round(ts[-1], digits)}


def schedule(names, rounds):
    """The windows in the order they are timed, round-major: [(round, name), ...] with every name once per round, in the given order,
    before the next round starts - so drift of a shared machine lands on every name alike."""
    return [(r, n) for r in range(rounds) for n in names]


def graph_of(fn, reps, warm=2):
    """`warm` eager calls on a side stream (capture-safe: it waits for the current stream and is waited for), a synchronise, `reps`
    calls captured into one graph, one untimed replay, a synchronise -> the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def _window_ms(fn, n):
    """One event pair around n calls of fn, synchronised: milliseconds per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def window_us(graph, reps, replays):
    """One event pair around `replays` replays of a graph of `reps` calls: microseconds per call."""
    return _window_ms(graph.replay, replays) / reps * 1e3


def time_calls(named, rounds, reps, replays, warm=2):
    """Time the callables of `named` (name -> callable) against each other: every graph is built first (``graph_of``), then the windows
    of ``schedule`` are walked -> {name: [microseconds per call, one entry per round]}.
    Each callable runs exactly warm + reps * (1 + rounds * replays) times."""
    require_gpu("time_calls")
    graphs = {n: graph_of(fn, reps, warm) for n, fn in named.items()}
    ts = {n: [] for n in named}
    for _, n in schedule(list(named), rounds):
        ts[n].append(window_us(graphs[n], reps, replays))
    return ts


def time_steps(step, rounds, replays, warm=5):
    """For a step that needs no capture here (a model after ``capture_graph``, or a call that cannot be captured): `warm` untimed
    steps, then one window of `replays` steps per round -> [milliseconds per step, one entry per round].  It runs warm + rounds * replays
    steps and no other."""
    require_gpu("time_steps")
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    return [_window_ms(step, replays) for _ in range(rounds)]


def emit(tag, obj):
    """The child's side of ``alternate_trees``: one tagged JSON line on stdout."""
    print(tag + " " + json.dumps(obj), flush=True)


def alternate_trees(script, trees, rounds, tag, child_args, timeout):
    """This tree against another checkout.  In every round, for every (label, root, extra_args) of `trees`, one FRESH process
    `python script --child root *extra_args *child_args` runs to its end before the next starts; the last line of its stdout that begins
    with `tag` is a JSON object (``emit``) whose values are appended to runs[label + ":" + name] -> runs.
    A child that exits non-zero or outlives `timeout` seconds ends everything at once: nothing more is started after a failure."""
    runs = {}
    for r, (label, root, extra) in schedule(trees, rounds):
        cmd = [sys.executable, script, "--child", root, *extra, *child_args]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
            status, so, se = p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            status = f"none, killed after {timeout} s"
            so, se = (s.decode(errors="replace") if isinstance(s, bytes) else s or "" for s in (e.stdout, e.stderr))
        if status != 0:
            sys.exit(f"{label} tree, round {r}: exit {status}\n{so[-2000:]}\n{se[-2000:]}")
        line = [ln for ln in so.splitlines() if ln.startswith(tag + " ")][-1]
        for name, v in json.loads(line[len(tag) + 1:]).items():
            runs.setdefault(f"{label}:{name}", []).append(v)
    return runs


def bleed_batch(B, H, W, in_channels, generator):
    """A synthetic labelled batch, built on the host from the seeded generator -> (x [B,H,W,in_channels] in [-1, 1], one-hot y [B,H,W,3])
    on the device: a bleed class (2) of about 1.5 % of the pixels inside a band of class 1."""
    x = torch.randn(B, H, W, in_channels, generator=generator).clamp_(-1, 1).cuda()
    lab = torch.zeros(B, H, W, dtype=torch.long)
    lab[:, H // 3:H // 3 + H // 8, W // 3:W // 3 + W // 8] = 2
    lab[:, H // 4:3 * H // 4, :][lab[:, H // 4:3 * H // 4, :] == 0] = 1
    return x, torch.nn.functional.one_hot(lab, 3).float().cuda()


def write_json(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
