"""CPU tests of gradient accumulation: argument validation, the order in which ``step.TrainStepDriver`` calls its
hooks with N micro-batches per optimiser step (driven with plain torch arithmetic, as tests/test_cpu_host.py drives the step order), a
world-size-2 gloo run, and the refusal of ``save`` while micro-steps are pending.  The kernel itself is tests/test_gpu_accumulate.py's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import accumulate_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the binding
def test_the_fourth_header_parses_and_the_library_exports_its_symbol():
    import ctypes as C
    from ultrasound_modeling_amd import _abi, _lib as L
    path = os.path.join(ROOT, "include", "usseg_accumulate.h")
    assert L.GRAD_ACC_HEADER_PATH == path
    abi = _abi.parse(open(path).read(), path)
    assert tuple(abi.protos) == ("usseg_grad_accumulate",) == L.GRAD_ACC_SYMBOLS and not abi.structs and not abi.consts
    assert abi.protos["usseg_grad_accumulate"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p])
    lib = L.load()                                         # the binding is generated from the header, and load() binds it
    fn = lib.usseg_grad_accumulate
    assert (fn.restype, list(fn.argtypes)) == L.GRAD_ACC_ABI.protos["usseg_grad_accumulate"]
    assert "usseg_grad_accumulate" not in L.EXPORTED_SYMBOLS and "usseg_grad_accumulate" not in L._PROTOS    # usseg.h's table is as it was


def test_bad_arguments_are_refused_before_any_launch():
    from ultrasound_modeling_amd import _lib as L
    lib = L.load()
    fn = lib.usseg_grad_accumulate                         # every argument is checked before a launch: none of these touches a device
    assert fn(None, None, 0, 1, 2.0, None) == 0                                                             # n == 0: nothing to do
    assert fn(None, None, 8, 0, 1.0, None) == -1 and b"null pointer" in lib.usseg_last_error()
    assert fn(16, 64, -1, 0, 1.0, None) == -1 and fn(16, 68, 8, 0, 1.0, None) == -1 and b"aligned" in lib.usseg_last_error()
    assert fn(16, 32, 8, 0, 1.0, None) == -1 and b"overlap" in lib.usseg_last_error()                       # 8 floats from 16 reach 48
    assert fn(16, 64, 8, 2, 1.0, None) == -1 and fn(16, 64, 8, 1, 0.5, None) == -1 and b"divisor" in lib.usseg_last_error()


def test_the_timing_script_goes_through_the_timing_module():
    import subprocess
    src = open(os.path.join(ROOT, "tools", "time_accumulate.py")).read()
    assert "import timing" in src and "CUDAGraph()" not in src and "enable_timing=True" not in src      # no timing primitive of its own
    assert "timing.time_calls(" in src and "timing.alternate_trees(" in src and "timing.time_steps(" in src
    p = subprocess.run([sys.executable, os.path.join("tools", "time_accumulate.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and "usage" in p.stdout.lower(), (p.stdout[-1000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad", [0, -1, True, False, 2.0, "2", [2], 2 ** 24 + 1])
def test_accumulate_must_be_a_positive_integer(bad):
    from ultrasound_modeling_amd.flat import accumulate_config
    from ultrasound_modeling_amd.SwinTransformer import SwinTransformerModel
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    with pytest.raises(ValueError, match="accumulate"):
        accumulate_config(bad)
    with pytest.raises(ValueError, match="accumulate"):
        TransUNet(img_size=(64, 128), batch_size=2, in_channels=1, accumulate=bad)
    with pytest.raises(ValueError, match="accumulate"):
        SwinTransformerModel(model_name="t", img_size=(64, 64), in_chans=1, embed_dim=32, depths=[2, 2], num_heads=[2, 4], window_size=4, accumulate=bad)
    with pytest.raises(ValueError, match="accumulate"):        # refused before any device is touched: the same error with and without a GPU
        VisionTransformer(batch_size=2, img_size=(32, 32), in_channels=1, accumulate=bad)
    with pytest.raises(ValueError, match="accumulate"):
        ResNest(64, 64, 1, 3, 3, accumulate=bad)


def test_accumulate_values():
    from ultrasound_modeling_amd.flat import accumulate_config
    assert accumulate_config(None) == 1 and accumulate_config(1) == 1 and accumulate_config(3) == 3 and accumulate_config(np.int64(4)) == 4
    assert accumulate_config(2 ** 24) == 2 ** 24 == int(np.float32(2 ** 24))       # the largest N: (float)N is still N
    with pytest.raises(ValueError, match=r"2\^24"):
        accumulate_config(2 ** 24 + 1)                                              # np.float32(2^24 + 1) would be 2^24
    assert type(accumulate_config(np.int64(4))) is int


def _flat_params():
    import torch.nn as nn
    from ultrasound_modeling_amd.flat import FlatParams

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.arange(13, dtype=torch.float32))
    return FlatParams(Net(), "cpu")


def test_none_and_one_construct_no_accumulator():
    from ultrasound_modeling_amd.flat import AdamClip
    fp = _flat_params()
    plain = AdamClip(fp)
    for off in (None, 1):
        opt = AdamClip(fp, accumulate=off)
        assert opt.acc is None and opt.accumulate_steps == 1
        assert len(opt.state_tensors()) == len(plain.state_tensors()) and set(opt.state_dict()) == set(plain.state_dict())
        with pytest.raises(RuntimeError, match="accumulate"):
            opt.accumulate(True)                                   # nothing to accumulate into: an error, not a silent no-op
    opt = AdamClip(fp, accumulate=3)
    assert opt.accumulate_steps == 3 and opt.acc.shape == fp.grad.shape and opt.acc.dtype == torch.float32 and not opt.acc.any()
    assert opt.acc.data_ptr() != fp.grad.data_ptr()
    assert any(t is opt.acc for t in opt.state_tensors())          # the capture warm-up puts it back with the rest of the state
    assert set(opt.state_dict()) == set(plain.state_dict())        # a checkpoint never holds it: save refuses while anything is pending


# ------------------------------------------------------------------------------------------------ the step order
class _Flat:
    def __init__(self, n):
        self.flat, self.grad, self.total = torch.zeros(n), torch.zeros(n), n


class _Opt:
    """flat.AdamClip's interface in fp32 torch-CPU arithmetic, every call recorded; ``accumulate`` is the kernel's restatement."""

    def __init__(self, flat, n, log):
        self.flat, self.accumulate_steps, self.calls = flat, n, log
        self.acc = torch.zeros_like(flat.grad) if n > 1 else None
        self.step = 0

    def accumulate(self, finish):
        self.calls.append(("accumulate", bool(finish)))
        if finish:
            acc, g = R.finish(self.acc.numpy(), self.flat.grad.numpy(), self.accumulate_steps)
            self.flat.grad.copy_(torch.from_numpy(g))
        else:
            acc = R.micro(self.acc.numpy(), self.flat.grad.numpy())
        self.acc.copy_(torch.from_numpy(acc))

    def clip_local(self):
        self.calls.append("clip_local")
        self.flat.grad.mul_(1.0 / max(float(self.flat.grad.norm()), 1.0))

    def advance(self):
        self.calls.append("advance")
        self.step += 1

    def apply_range(self, lo, hi, clip=0.0):
        self.calls.append(("adam", lo, hi))
        self.seen = self.flat.grad.clone()                 # the gradient the update reads
        self.flat.flat[lo:hi].sub_(0.5 * self.flat.grad[lo:hi])

    def apply(self, already_clipped=False):
        self.calls.append(("apply", already_clipped))
        self.advance()
        self.apply_range(0, self.flat.total)


def _make_net(n_acc, size=8):
    from ultrasound_modeling_amd.step import TrainStepDriver

    class Net(TrainStepDriver):
        """The PRODUCT's step driver; the "model" has gradient x (the batch itself), so every expected number is in the test."""

        def __init__(self):
            self.calls = []
            self.flat = _Flat(size)
            self.optimizer = _Opt(self.flat, n_acc, self.calls)
            self.grad_sync = None

        def _zero_grad(self):
            self.calls.append("zero")
            self.flat.grad.zero_()

        def _forward_backward(self, x, y):
            self.calls.append("fwd_bwd")
            self.flat.grad.add_(x)
            return x

        def _repack(self):
            self.calls.append("repack")

        def train_step(self, x, y=None):
            return torch.zeros(()), self._train_body(x, y)
    return Net()


def _batches(k, size=8):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(size, generator=g) * (3.0 ** i) for i in range(k)]


MICRO = ["zero", "fwd_bwd", ("accumulate", False)]


@pytest.mark.parametrize("n", [2, 3])
def test_one_update_per_group_of_n(n):
    net, xs = _make_net(n), _batches(2 * n)
    for i, x in enumerate(xs):
        assert net.pending_micro_steps == i % n
        net.train_step(x)
    assert net.pending_micro_steps == 0 and net.accumulate == n
    finishing = ["zero", "fwd_bwd", ("accumulate", True), ("apply", False), "advance", ("adam", 0, 8), "repack"]
    assert net.calls == (MICRO * (n - 1) + finishing) * 2          # no clip, exchange, Adam, repack or advance inside a group
    assert net.optimizer.step == 2
    want = R.group([x.numpy() for x in xs[n:]], n)                 # the second group starts from a zero accumulator
    assert R.same_bits(net.optimizer.seen.numpy(), want).all() and not net.optimizer.acc.any()
    w = np.zeros(8, np.float32)
    for k in range(2):
        w = w - np.float32(0.5) * R.group([x.numpy() for x in xs[k * n:(k + 1) * n]], n)
    assert np.array_equal(net.flat.flat.numpy(), w)


def test_clip_local_only_on_the_finishing_micro_step_and_after_accumulate():
    net, xs = _make_net(3), _batches(3)
    syncs = []
    net.grad_sync = lambda g: syncs.append(g.clone())
    for x in xs:
        net.train_step(x)
    assert net.calls == MICRO * 2 + ["zero", "fwd_bwd", ("accumulate", True), "clip_local", ("apply", True), "advance", ("adam", 0, 8), "repack"]
    mean = torch.from_numpy(R.group([x.numpy() for x in xs], 3))
    assert len(syncs) == 1 and torch.equal(syncs[0], mean * (1.0 / max(float(mean.norm()), 1.0)))     # the exchange carries the CLIPPED MEAN


def test_chunked_exchange_runs_once_per_group():
    net, xs = _make_net(2), _batches(4)

    class Sync:
        n = 0

        def __call__(self, g):
            raise AssertionError("the chunked form is used")

        def chunks(self, g):
            Sync.n += 1
            for lo, hi in ((0, 4), (4, 8)):
                yield lo, hi, (lambda: None)
    net.grad_sync = Sync()
    for x in xs:
        net.train_step(x)
    assert Sync.n == 2 and net.calls.count("advance") == 2 and net.calls.count("repack") == 2
    assert [c for c in net.calls if isinstance(c, tuple) and c[0] == "adam"] == [("adam", 0, 4), ("adam", 4, 8)] * 2


def test_accumulate_one_and_none_run_todays_order():
    net, xs = _make_net(1), _batches(2)
    for x in xs:
        net.train_step(x)
    assert net.calls == ["zero", "fwd_bwd", ("apply", False), "advance", ("adam", 0, 8), "repack"] * 2
    assert net.pending_micro_steps == 0
    net = _make_net(1)
    del net.optimizer.accumulate_steps                 # an optimiser that knows nothing of accumulation (bench.py's CPU stand-in) is N = 1
    net.train_step(_batches(1)[0])
    net.flush_step()
    assert net.calls == ["zero", "fwd_bwd", ("apply", False), "advance", ("adam", 0, 8), "repack"] and net.accumulate == 1


def test_flush_step_finishes_a_short_group_and_still_divides_by_n():
    net, xs = _make_net(3), _batches(2)
    net.flush_step()                                   # nothing pending: nothing happens
    assert net.calls == [] and net.optimizer.step == 0
    net.train_step(xs[0])
    net.train_step(xs[1])
    assert net.pending_micro_steps == 2
    net.flush_step()
    assert net.pending_micro_steps == 0 and net.optimizer.step == 1
    assert net.calls == MICRO * 2 + ["zero", ("accumulate", True), ("apply", False), "advance", ("adam", 0, 8), "repack"]     # no forward pass
    want = R.group([xs[0].numpy(), xs[1].numpy(), np.zeros(8, np.float32)], 3)
    assert R.same_bits(net.optimizer.seen.numpy(), want).all() and not net.optimizer.acc.any()
    n_calls = len(net.calls)
    net.flush_step()
    assert len(net.calls) == n_calls and net.optimizer.step == 1


def test_empty_step_counts_as_a_micro_step():
    net, xs = _make_net(2), _batches(2)
    net.empty_step()                                   # first of the group: a zero gradient into the accumulator, nothing else
    assert net.calls == ["zero", ("accumulate", False)] and net.pending_micro_steps == 1
    net.train_step(xs[0])
    assert net.optimizer.step == 1 and net.pending_micro_steps == 0
    assert R.same_bits(net.optimizer.seen.numpy(), R.group([np.zeros(8, np.float32), xs[0].numpy()], 2)).all()
    net.train_step(xs[1])
    net.empty_step()                                   # second of the group: it finishes it
    assert net.optimizer.step == 2 and net.pending_micro_steps == 0 and net.calls[-6:] == ["zero", ("accumulate", True), ("apply", False),
                                                                                            "advance", ("adam", 0, 8), "repack"]
    assert R.same_bits(net.optimizer.seen.numpy(), R.group([xs[1].numpy(), np.zeros(8, np.float32)], 2)).all()


def test_training_step_inside_averaged_weights_still_raises_for_micro_steps():
    net = _make_net(2)
    net._averaged = True
    with pytest.raises(RuntimeError, match="averaged_weights"):
        net.train_step(_batches(1)[0])
    net._pending = 1
    with pytest.raises(RuntimeError, match="averaged_weights"):
        net.flush_step()


def test_save_with_pending_micro_steps_raises(tmp_path):
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    net = _make_net(3)
    net.train_step(_batches(1)[0])
    for save in (VisionTransformer.save, ResNest.save_params):         # the models' own save code, on a driver with one micro-step pending
        with pytest.raises(RuntimeError, match=r"1 of 3 micro-steps are pending.*flush_step"):
            save(net, str(tmp_path / "m.pt"))
    assert not (tmp_path / "m.pt").exists()
    net.flush_step()
    net._no_pending("save")                                            # flushed: save goes on


def test_load_with_pending_micro_steps_raises(tmp_path):
    """The accumulator holds gradients of the weights a load would replace: the models' load paths refuse before they read anything."""
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    net = _make_net(2)
    net.train_step(_batches(1)[0])
    missing = str(tmp_path / "never_read.pt")
    for load, arg in ((VisionTransformer.load, missing), (VisionTransformer.load_params, {}), (ResNest.load_params_file, missing),
                      (ResNest.load_params, {})):
        with pytest.raises(RuntimeError, match=r"1 of 2 micro-steps are pending.*flush_step"):
            load(net, arg)
    assert net.pending_micro_steps == 1 and net.optimizer.acc.abs().max() > 0       # the group is as it was


# ------------------------------------------------------------------------------------------------ world_size-2 gloo
def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from ultrasound_modeling_amd.MainParallel import MirroredTrainer, init_distributed
    init_distributed("gloo")
    torch.set_num_threads(1)
    net = _make_net(2)
    net.flat.flat.fill_(float(rank + 1))                               # ranks start different; rank 0's weights are mirrored
    net.modules = lambda: []
    MirroredTrainer(net)
    inner, exchanges = net.grad_sync, []

    class Counting:
        chunks = None

        def __call__(self, g):
            exchanges.append(len(net.calls))
            inner(g)
    net.grad_sync = Counting()
    g = torch.Generator().manual_seed(11 + rank)
    xs = [torch.randn(8, generator=g) for _ in range(5)]
    # group 1: two batches; group 2: rank 1 holds no image in the first micro-step; group 3: one micro-step, flushed
    net.train_step(xs[0], None)
    net.train_step(xs[1], None)
    if rank == 1:
        net.empty_step()
    else:
        net.train_step(xs[2], None)
    net.train_step(xs[3], None)
    net.train_step(xs[4], None)
    assert net.pending_micro_steps == 1 and len(exchanges) == 2
    net.flush_step()
    assert net.pending_micro_steps == 0
    torch.save({"w": net.flat.flat.clone(), "exchanges": len(exchanges), "steps": net.optimizer.step, "xs": xs,
                "clips": net.calls.count("clip_local")}, os.path.join(tmp, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_one_exchange_per_optimiser_step(tmp_path):
    """Five micro-steps with N = 2 and a flush: three optimiser steps, so three gradient exchanges and three per-replica clips - not five;
    a rank that holds no image inside a group stays in step, and the ranks' weights stay identical."""
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for r in (r0, r1):
        assert r["exchanges"] == 3 and r["steps"] == 3 and r["clips"] == 3
    assert torch.equal(r0["w"], r1["w"])
    # the same numbers from the restatement: per rank the clipped group mean, summed over the ranks in fp32, w -= 0.5 * that
    z = np.zeros(8, np.float32)
    groups = [lambda xs, rank: [xs[0], xs[1]], lambda xs, rank: [z if rank == 1 else xs[2], xs[3]], lambda xs, rank: [xs[4], z]]
    w = np.ones(8, np.float32)
    for grp in groups:
        total = np.zeros(8, np.float32)
        for rank, r in enumerate((r0, r1)):
            mean = torch.from_numpy(R.group([np.asarray(t) for t in grp(r["xs"], rank)], 2))
            total = total + mean.mul(1.0 / max(float(mean.norm()), 1.0)).numpy()
        w = w - np.float32(0.5) * total
    assert np.array_equal(r0["w"].numpy(), w)
