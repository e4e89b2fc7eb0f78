"""GPU tests of the device-resident learning-rate / weight-decay schedule and the AdamW update.

The kernels are pinned against the EXISTING ones, so no NumPy emulation of FMA contraction is needed:
  * ``usseg_adamw_step`` with wd = 0 and no mask == ``usseg_adam_clip_step`` bit for bit (clip on / off, n = 0..3 mod 4, sub-ranges
    at ``even_chunks`` offsets, planted +-0, subnormals and large values); with wd > 0 == "host-side p - wd*p in float32, then
    usseg_adam_clip_step"; excluded elements == the undecayed path;
  * ``usseg_sched_advance`` / ``usseg_sumsq_sched_advance`` over steps crossing every boundary == ``usseg_adam_advance(v[piece])``;
and the model paths: eager == captured-graph replay == an eager run whose host sets the rates at the boundaries, a rate set after
``capture_graph`` reaching the replay, the chunked data-parallel update, Arch A, checkpoints, and the untouched default path.
"""
import os

import numpy as np
import pytest
import torch

import usseg_oracle as O
from ultrasound_modeling_amd import ops
from ultrasound_modeling_amd.schedules import PiecewiseConstantDecay
from ultrasound_modeling_amd.step import even_chunks

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-7


def _table(boundaries, lr, wd):
    t = np.zeros(48, dtype=np.int32)
    t[0] = len(lr)
    t[1:1 + len(boundaries)] = boundaries
    t[16:16 + len(lr)] = np.asarray(lr, dtype=np.float32).view(np.int32)
    t[32:32 + len(wd)] = np.asarray(wd, dtype=np.float32).view(np.int32)
    return torch.from_numpy(t).to(DEV)


def _planted(n, seed):
    """p, g, m, v with +-0, subnormals and large magnitudes planted among normal values."""
    gen = torch.Generator().manual_seed(seed)
    p, g, m = (torch.randn(n, generator=gen) * 0.1 for _ in range(3))
    v = torch.rand(n, generator=gen) * 1e-3
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, 1e-38, 65504.0])
    g_special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e18, -1e18, 1e-38, 65504.0])     # the squared norm stays finite
    for t, sp in ((p, special), (g, g_special), (m, special)):
        idx = torch.randint(0, n, (min(n, 64),), generator=gen)
        t[idx] = sp[torch.randint(0, len(sp), (len(idx),), generator=gen)]
    idx = torch.randint(0, n, (min(n, 32),), generator=gen)
    v[idx] = torch.tensor([0.0, 1e-40, 1e30, 1e-38])[torch.randint(0, 4, (len(idx),), generator=gen)]
    return [t.to(DEV) for t in (p, g, m, v)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(a, b, what):
    if not torch.equal(_bits(a), _bits(b)):
        d = (_bits(a) != _bits(b))
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ in their bits")


def _lr_t(step, lr):
    s, l = torch.tensor([step], dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    ops.adam_advance(s, l, lr, B1, B2)
    return l


# ---------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("n", [4096, 4097, 4098, 4099, 1, 2, 3, 5123])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_adamw_without_decay_equals_adam(n, clip):
    p, g, m, v = _planted(n, seed=n)
    sumsq = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.sumsq(g, sumsq)
    lr_t, wd_t = _lr_t(4, 1e-3), torch.zeros(1, device=DEV)
    ref = [t.clone() for t in (p, g, m, v)]
    ops.adam_clip_step(ref[0], ref[1], ref[2], ref[3], sumsq, clip, lr_t, B1, B2, EPS)
    ops.adamw_step(p, g, m, v, sumsq, clip, lr_t, wd_t, None, B1, B2, EPS)
    torch.cuda.synchronize()
    for a, b, k in zip((p, m, v), (ref[0], ref[2], ref[3]), "pmv"):
        _assert_bits(a, b, f"n={n} clip={clip} {k}")


@pytest.mark.parametrize("n", [3 * 1024 + 1, 5 * 1024 + 3, 4 * 1024])
def test_adamw_on_even_chunk_ranges_equals_one_adam_launch(n):
    p, g, m, v = _planted(n, seed=100 + n)
    sumsq = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.sumsq(g, sumsq)
    lr_t, wd_t = _lr_t(1, 1e-2), torch.zeros(1, device=DEV)
    ref = [t.clone() for t in (p, g, m, v)]
    ops.adam_clip_step(ref[0], ref[1], ref[2], ref[3], sumsq, 1.0, lr_t, B1, B2, EPS)
    ranges = even_chunks(n, 4)
    assert len(ranges) > 1 and all(lo % 1024 == 0 for lo, _ in ranges)
    for lo, hi in ranges:
        ops.adamw_step(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], sumsq, 1.0, lr_t, wd_t, None, B1, B2, EPS)
    torch.cuda.synchronize()
    for a, b, k in zip((p, m, v), (ref[0], ref[2], ref[3]), "pmv"):
        _assert_bits(a, b, f"chunks n={n} {k}")


@pytest.mark.parametrize("n", [4099, 8192])
@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_adamw_decay_equals_host_decay_then_adam(n, clip):
    wd = 3e-2
    p, g, m, v = _planted(n, seed=7 * n)
    sumsq = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.sumsq(g, sumsq)
    lr_t = _lr_t(2, 1e-3)
    wd_t = torch.tensor([wd], dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(n)
    mask = (torch.rand(n, generator=gen) > 0.3).to(torch.uint8)
    pc = p.cpu()
    decayed = (pc - torch.tensor(wd, dtype=torch.float32) * pc).to(DEV)      # two float32 roundings
    ref_d = [decayed, g.clone(), m.clone(), v.clone()]                        # every element decayed
    ref_u = [t.clone() for t in (p, g, m, v)]                                 # no element decayed
    for r in (ref_d, ref_u):
        ops.adam_clip_step(r[0], r[1], r[2], r[3], sumsq, clip, lr_t, B1, B2, EPS)
    all_ = [t.clone() for t in (p, g, m, v)]
    ops.adamw_step(all_[0], all_[1], all_[2], all_[3], sumsq, clip, lr_t, wd_t, None, B1, B2, EPS)
    masked = [t.clone() for t in (p, g, m, v)]
    ops.adamw_step(masked[0], masked[1], masked[2], masked[3], sumsq, clip, lr_t, wd_t, mask.to(DEV), B1, B2, EPS)
    torch.cuda.synchronize()
    _assert_bits(all_[0], ref_d[0], "decayed p")
    _assert_bits(all_[2], ref_d[2], "m")
    _assert_bits(all_[3], ref_d[3], "v")
    keep = mask.bool().to(DEV)
    want = torch.where(keep, ref_d[0], ref_u[0])
    _assert_bits(masked[0], want, "masked p")
    assert not torch.equal(_bits(ref_d[0]), _bits(ref_u[0])), "the decay must change something"


def test_sched_advance_equals_adam_advance_across_every_boundary():
    bnd, lr, wd = [2, 4, 7], [1e-2, 3e-3, 1e-3, 3e-4], [1e-4, 3e-5, 0.0, 1e-6]
    table = _table(bnd, lr, wd)
    s = PiecewiseConstantDecay(bnd, lr)
    g = torch.randn(10000, device=DEV)
    ref_sum = torch.zeros(ops.ACC_FLOATS, device=DEV)
    ops.sumsq(g, ref_sum)
    for x in range(10):
        piece = s.piece(x)
        want = _lr_t(x, lr[piece])
        for fused in (False, True):
            step = torch.tensor([x], dtype=torch.int32, device=DEV)
            lr_t, wd_t = torch.zeros(1, device=DEV), torch.full((1,), -1.0, device=DEV)
            if fused:
                acc = torch.zeros(ops.ACC_FLOATS, device=DEV)
                ops.sumsq_sched_advance(g, acc, step, table, lr_t, wd_t, B1, B2)
                _assert_bits(acc[:1], ref_sum[:1], "sumsq_sched_advance's norm")
            else:
                ops.sched_advance(step, table, lr_t, wd_t, B1, B2)
            torch.cuda.synchronize()
            assert int(step.item()) == x + 1
            _assert_bits(lr_t, want, f"x={x} fused={fused} lr_t")
            assert wd_t.item() == np.float32(wd[piece]), (x, fused)


# ---------------------------------------------------------------------------------------------------- model level
BND = [1, 3]
LRS = PiecewiseConstantDecay(BND, [1e-3, 5e-4, 2e-4])
WDS = PiecewiseConstantDecay(BND, [1e-2, 5e-3, 1e-3])
NSTEPS = 6


def _batches(n, B=2, H=64, W=64):
    return [O.synthetic_batch(B, H, W, 1, seed=70 + i) for i in range(n)]


def _arch_b(seed=3, **kw):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True).items()}
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1, **kw)
    net.load_params(P)
    return net


def _state(net):
    torch.cuda.synchronize()
    o = net.optimizer
    return dict(p=net.flat.flat.clone(), m=o.m.clone(), v=o.v.clone(), step=int(o.step_dev.item()))


def _assert_same_state(a, b, what):
    assert a["step"] == b["step"], (what, a["step"], b["step"])
    for k in ("p", "m", "v"):
        _assert_bits(a[k], b[k], f"{what}: {k}")


def _host_rates(net, x):
    """The eager twin of the schedule: the host sets the rates of step x's piece before that step."""
    if x in (0, BND[0] + 1, BND[1] + 1):
        net.optimizer.set_learning_rate(float(LRS(x)))
        net.optimizer.set_weight_decay(float(WDS(x)))


@pytest.fixture(scope="module")
def scheduled_run():
    """Arch B, eager, schedule + AdamW: the state after every step."""
    net = _arch_b(learning_rate=LRS, weight_decay=WDS, adamw=True)
    assert net.optimizer.scheduled
    states = []
    for x, y in _batches(NSTEPS):
        net.train_step(x, y.float())
        states.append(_state(net))
    return states


def test_scheduled_graph_and_host_set_rates_equal_eager(scheduled_run):
    bs = _batches(NSTEPS)
    graph = _arch_b(learning_rate=LRS, weight_decay=WDS, adamw=True)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    host = _arch_b(learning_rate=1.0, weight_decay=1.0, adamw=True)
    for i, (x, y) in enumerate(bs):
        graph.train_step(x, y.float())
        _host_rates(host, i)
        host.train_step(x, y.float())
        _assert_same_state(_state(graph), scheduled_run[i], f"graph step {i}")
        _assert_same_state(_state(host), scheduled_run[i], f"host-set step {i}")
    assert scheduled_run[-1]["step"] == NSTEPS
    plain = _arch_b(learning_rate=1e-3)
    for x, y in bs[:2]:
        plain.train_step(x, y.float())
    assert not torch.equal(_state(plain)["p"], scheduled_run[1]["p"]), "the decay must move the weights"


def test_set_rates_after_capture_reach_the_replay(scheduled_run):
    bs = _batches(NSTEPS)
    graph = _arch_b(learning_rate=1.0, weight_decay=1.0, adamw=True)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    for i, (x, y) in enumerate(bs):
        _host_rates(graph, i)
        graph.train_step(x, y.float())
        _assert_same_state(_state(graph), scheduled_run[i], f"replay step {i}")
    assert graph.optimizer.current_learning_rate() == float(LRS(NSTEPS))


@pytest.fixture(scope="module")
def rccl_world1():
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        port = 29300 + os.getpid() % 300
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)   # "nccl" is RCCL on ROCm
        created = True
    yield dist
    if created:
        dist.destroy_process_group()


def test_chunked_data_parallel_update_equals_unchunked(rccl_world1, scheduled_run):
    from ultrasound_modeling_amd.MainParallel import MirroredTrainer
    one = _arch_b(learning_rate=LRS, weight_decay=WDS, adamw=True)
    four = _arch_b(learning_rate=LRS, weight_decay=WDS, adamw=True)
    t1, t4 = MirroredTrainer(one, force=True, chunks=1), MirroredTrainer(four, force=True, chunks=4)
    assert getattr(four.grad_sync, "chunks", None) is not None and getattr(one.grad_sync, "chunks", None) is None
    for i, (x, y) in enumerate(_batches(NSTEPS)):
        t1.train_step(x, y.float())
        t4.train_step(x, y.float())
        _assert_same_state(_state(four), _state(one), f"chunked step {i}")
        _assert_same_state(_state(one), scheduled_run[i], f"data-parallel step {i}")


def test_arch_a_graph_equals_eager_with_schedule_and_decay():
    from ultrasound_modeling_amd.TBI_ResNest import ResNest

    def make():
        P = {k: v.float().double() for k, v in O.init_archA_params(channel=1, radix=3, kpaths=4, seed=4, perturb=True).items()}
        net = ResNest(64, 64, 1, 3, ksize=3, radix=3, kpaths=4, learning_rate=10 * LRS, weight_decay=WDS)
        net.load_params(P)
        return net
    eager, graph = make(), make()
    bs = _batches(4)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    for i, (x, y) in enumerate(bs):
        lm0, _, p0 = eager.step(x, y.float(), train=True)
        lm1, _, p1 = graph.step(x, y.float(), train=True)
        torch.cuda.synchronize()
        assert torch.equal(lm0, lm1) and torch.equal(p0, p1), i
        _assert_same_state(_state(eager), _state(graph), f"Arch A step {i}")


def test_checkpoint_resumes_the_schedule(tmp_path, scheduled_run):
    bs = _batches(NSTEPS)
    a = _arch_b(learning_rate=LRS, weight_decay=WDS, adamw=True)
    for x, y in bs[:2]:
        a.train_step(x, y.float())
    a.save(str(tmp_path / "s.pt"))
    b = _arch_b(seed=9, learning_rate=LRS, weight_decay=WDS, adamw=True)
    b.load(str(tmp_path / "s.pt"))
    for i in range(2, NSTEPS):
        x, y = bs[i]
        b.train_step(x, y.float())
        _assert_same_state(_state(b), scheduled_run[i], f"resumed step {i}")
    old = _arch_b(learning_rate=1e-3)                  # an old-format checkpoint (no __adam_sched__) loads as before
    old.train_step(bs[0][0], bs[0][1].float())
    old.save(str(tmp_path / "old.pt"))
    assert "__adam_sched__" not in torch.load(str(tmp_path / "old.pt"), weights_only=True)
    c = _arch_b(seed=9, learning_rate=LRS, weight_decay=WDS, adamw=True)
    c.load(str(tmp_path / "old.pt"))
    _assert_same_state(_state(c), _state(old), "old-format load")
    assert c.optimizer.lr == LRS and c.optimizer.weight_decay == WDS


def test_default_model_keeps_the_fixed_rate_kernels(monkeypatch):
    net = _arch_b(learning_rate=1e-3)
    o = net.optimizer
    assert not o.scheduled and o.sched_dev is None and o.wd_t_dev is None
    assert set(o.state_dict()) == {"__adam_m__", "__adam_v__", "__adam_step__"}
    assert len(o.state_tensors()) == 4

    def forbidden(*a, **k):
        raise AssertionError("a default model launched a schedule kernel")
    for name in ("adamw_step", "sched_advance", "sumsq_sched_advance"):
        monkeypatch.setattr(ops, name, forbidden)
    x, y = _batches(1)[0]
    net.train_step(x, y.float())
    assert _state(net)["step"] == 1
    vit = _arch_b(learning_rate=1e-3, weight_decay=1e-4)          # weight_decay without adamw stays unused, as in the reference
    assert not vit.optimizer.scheduled
