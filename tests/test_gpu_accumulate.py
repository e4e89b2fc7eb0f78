"""GPU tests of gradient accumulation (include/usseg_accumulate.h ``usseg_grad_accumulate``).

  * the kernel, bit for bit against tests/accumulate_restatement.py: both behaviours from an arbitrary accumulator, and whole groups with
    N = 3 and N = 4, at flat lengths 8, 11 (the scalar tail), 1032 (a second workgroup with a short vector tail) and 2*4096*1024 + 1032
    (every workgroup of the capped grid takes two grid-stride trips and some a third), with -0.0, denormals, sums that round, overflow, one inf
    and one NaN among the inputs; after a finish the accumulator is all +0.0;
  * the smallest Arch B model of the GPU model tests (2 x 64x64x1): a group of N = 3 against a twin model whose gradient buffer receives the
    restated mean - weights, Adam moments and step counter bit for bit; N = 2 with ``batch_size=2`` against one step of a ``batch_size=4`` model
    on the concatenated batch; ``accumulate=1`` == ``None``; eager == captured replay over two groups; ``flush_step``; EMA once per group; the
    data-parallel order over an in-process RCCL group; ``save`` refuses while micro-steps are pending;
  * ``accumulate=`` on the other three models: the TransUNet variant, Arch A (fresh dropout masks per micro-step) and the Swin encoder.

Bounds of the ``batch_size=4`` comparison (nothing else here has a tolerance).  Every image is computed on its own whichever batch it
is in (per-sample LayerNorm, BatchNorm on its moving statistics); what differs is the order of the fp32 sums over the batch in the loss and in
the weight gradients.  For that the project has tests/test_gpu_topk.py::test_image_scope_does_not_depend_on_how_the_batch_is_split (two replicas
with half the batch each against one with all of it): flat gradients within U_BF16 = 2^-8 of the big gradient's norm, losses within 1e-5
relative - both taken over unchanged.  For the weights after the one step the project's one-step bar is
tests/test_gpu_model.py::test_train_step_parity's: the UPDATE within 0.15 in relative L2 (the first Adam step is ~lr*sign(g), so entries
whose gradient is at rounding level may flip) - taken over unchanged.  Per element there is no bar in the GPU model tests to take over, and the
update rule alone gives none worth asserting (with zero moments |lr_t * m / (sqrt(v) + eps)| < lr, so ANY two gradients leave the weights
within 2*lr of each other): the largest per-element difference is printed, not asserted.  Observed on an MI355X: the same loss to the last bit,
flat gradients 5.1e-8 apart, updates 2.3e-7 apart, largest weight difference 6.0e-8 - the taken-over bars are far looser than the code needs.
"""
import os

import numpy as np
import pytest
import torch

import accumulate_restatement as R
import usseg_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U_BF16 = 2.0 ** -8
LR = 1e-3
BIG = 2 * 4096 * 1024 + 1032


# ------------------------------------------------------------------------------------------------ the kernel
def _inputs(n, k, seed):
    """k fp32 vectors of length n over a wide range of exponents; the first eight elements are the special cases."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(k):
        v = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
        v[0] = -0.0                                                     # -0.0 + -0.0 stays -0.0; +0.0 + -0.0 is +0.0
        v[1] = np.float32(1e-45) * (j + 1)                              # denormals in, denormal sum, denormal quotient
        v[2] = np.float32(1.0) if j == 0 else np.float32(2.0 ** -24 * (2 * j - 1))     # 1 + 2^-24 is a tie, then sums that round
        v[3] = np.inf if j == 1 else v[3]                               # one inf (with finite partners: it stays inf)
        v[4] = np.nan if j == min(2, k - 1) else v[4]                   # one NaN
        v[5] = np.float32(3e38)                                         # the sum overflows to inf
        v[6] = np.float32(2.0 ** -126) if j == 0 else np.float32(0.0)   # the smallest normal: its quotient by N is a denormal
        v[7] = np.float32(-0.0) if j % 2 else np.float32(1.5)
        out.append(v)
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    ok = R.same_bits(got, want)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {i}: {got[i]!r} ({got.view(np.uint32)[i]:#010x}) "
                             f"vs {want[i]!r} ({np.asarray(want).view(np.uint32)[i]:#010x})")


def _all_plus_zero(t):
    return not bool(t.view(torch.int32).any().item())


@pytest.mark.parametrize("n", [8, 11, 1032, BIG])
def test_both_behaviours_from_any_accumulator(n):
    from ultrasound_modeling_amd import ops
    a, g = _inputs(n, 2, seed=n % 1000)
    a[0], a[7] = np.float32(-0.0), np.float32(-0.0)                     # a -0.0 in the accumulator meets -0.0 and +1.5
    acc, grad = _dev(a), _dev(g)
    ops.grad_accumulate(acc, grad, False, 3.0)
    _assert_bits(acc, R.micro(a, g), "micro-step: acc")
    _assert_bits(grad, g, "micro-step: grad is only read")
    assert np.signbit(acc.cpu().numpy()[0]) and np.isinf(acc.cpu().numpy()[3]) and np.isinf(acc.cpu().numpy()[5])
    for N in (3, 4):
        acc, grad = _dev(a), _dev(g)
        ops.grad_accumulate(acc, grad, True, float(N))
        _assert_bits(grad, R.finish(a, g, N)[1], f"finish N={N}: grad")
        assert _all_plus_zero(acc), f"finish N={N}: acc is not all +0.0"
    got = grad.cpu().numpy()
    assert np.signbit(got[0]) and got[0] == 0 and np.isinf(got[3]) and np.isnan(got[4]) and np.isinf(got[5])


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("n", [8, 11, 1032, BIG])
def test_group_of_n_micro_steps(n, N):
    from ultrasound_modeling_amd import ops
    gs = _inputs(n, N, seed=7 * N + n % 1000)
    acc = torch.zeros(n, dtype=torch.float32, device=DEV)
    for rep in range(2):                                                # the second group starts from the zero the first one left
        for j, g in enumerate(gs):
            grad = _dev(g)
            ops.grad_accumulate(acc, grad, j == N - 1, float(N))
        want = R.group(gs, N)
        _assert_bits(grad, want, f"group {rep} of N={N}, n={n}")
        assert _all_plus_zero(acc)
    assert np.isnan(want[4]) and np.isinf(want[3]) and want[1] != 0 and abs(want[1]) < 2.0 ** -126 and 0 < want[6] < 2.0 ** -126


def test_bad_arguments_are_refused():
    from ultrasound_modeling_amd import _lib, ops
    acc, grad = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    for a, g, fin, div in ((acc, acc, True, 2.0), (acc[1:9], grad[:8], True, 2.0), (acc, grad, True, 0.0), (acc[:12], acc[8:], False, 1.0)):
        with pytest.raises((_lib.UssegError, AssertionError)):
            ops.grad_accumulate(a, g, fin, div)
    ops.grad_accumulate(acc[:0], grad[:0], True, 2.0)                   # n = 0: no launch, no error


# ------------------------------------------------------------------------------------------------ Arch B, 2 x 64x64x1
def _arch_b(seed=3, batch_size=2, **kw):
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    P = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True).items()}
    net = VisionTransformer(batch_size=batch_size, img_size=(64, 64), in_channels=1, learning_rate=LR, **kw)
    net.load_params(P)
    return net


def _batches(n, B=2, W=64):
    return [(x, y.float()) for x, y in (O.synthetic_batch(B, 64, W, 1, seed=60 + i) for i in range(n))]


def _state(net):
    torch.cuda.synchronize()
    o = net.optimizer
    return dict(p=net.flat.flat.clone(), m=o.m.clone(), v=o.v.clone(), step=int(o.step_dev.item()))


def _assert_same_state(a, b, what):
    assert a["step"] == b["step"], (what, a["step"], b["step"])
    for k in ("p", "m", "v"):
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            d = (a[k].double() - b[k].double()).abs()
            raise AssertionError(f"{what}: {k} differs in {(d > 0).sum().item()} of {d.numel()} entries (max abs {d.max().item():.3e})")


def _twin_gradient(twin, x, y):
    """The micro-batch gradient of a model WITHOUT accumulation that holds the same weights -> (flat gradient, loss, probabilities)."""
    probs = twin._grad_body(twin._prep_x(x), twin._prep_y(y))
    return twin.flat.grad.clone(), twin._loss[0].clone(), probs


def _twin_update(twin, grads, n):
    twin.flat.grad.copy_(torch.from_numpy(R.group([g.cpu().numpy() for g in grads], n)).to(DEV))
    twin._update_body()


def test_group_of_three_equals_the_restated_mean_in_a_twin():
    net, twin = _arch_b(accumulate=3), _arch_b()
    assert net.accumulate == 3 and twin.accumulate == 1 and twin.optimizer.acc is None
    start = _state(net)
    grads = []
    for i, (x, y) in enumerate(_batches(3)):
        g, loss_t, probs_t = _twin_gradient(twin, x, y)
        grads.append(g)
        assert net.pending_micro_steps == i
        loss, probs = net.train_step(x, y)
        torch.cuda.synchronize()
        assert loss.item() == loss_t.item() and torch.equal(probs, probs_t), f"micro-step {i}: loss / probabilities are the micro-batch's"
        if i < 2:
            _assert_same_state(_state(net), start, f"micro-step {i} must not touch weights, moments or the step counter")
    assert net.pending_micro_steps == 0
    _twin_update(twin, grads, 3)
    _assert_same_state(_state(net), _state(twin), "a group of 3")
    assert _state(net)["step"] == 1 and _all_plus_zero(net.optimizer.acc)
    _assert_bits(net.flat.grad, R.group([g.cpu().numpy() for g in grads], 3), "the gradient buffer holds the group's mean")


def test_two_micro_batches_against_one_step_of_the_big_batch():
    """Bounds: module docstring."""
    net, big = _arch_b(accumulate=2, batch_size=2), _arch_b(batch_size=4)
    x, y = O.synthetic_batch(4, 64, 64, 1, seed=70)
    y = y.float()
    before = net.flat.flat.clone()
    assert torch.equal(before, big.flat.flat)
    l1, _ = net.train_step(x[:2], y[:2])
    l1 = l1.item()
    l2, _ = net.train_step(x[2:], y[2:])
    lb, _ = big.train_step(x, y)
    torch.cuda.synchronize()
    mean_loss, lb = 0.5 * (l1 + l2.item()), lb.item()
    g, gb = net.flat.grad.double(), big.flat.grad.double()              # (the buffers keep the step's unclipped gradient)
    e_g = ((g - gb).norm() / gb.norm()).item()
    d, db = (net.flat.flat - before).double(), (big.flat.flat - before).double()
    e_u, e_max = ((d - db).norm() / db.norm()).item(), (net.flat.flat - big.flat.flat).abs().max().item()
    print(f"mean micro loss {mean_loss:.7f} vs big-batch loss {lb:.7f} (rel {abs(mean_loss - lb) / lb:.2e}); flat gradient rel {e_g:.3e}; "
          f"update rel {e_u:.3e}; largest weight difference {e_max:.3e} (lr {LR})")
    assert abs(mean_loss - lb) <= 1e-5 * lb
    assert gb.norm().item() > 0 and e_g <= U_BF16
    assert e_u < 0.15
    assert int(net.optimizer.step_dev.item()) == int(big.optimizer.step_dev.item()) == 1


def test_accumulate_one_is_none():
    one, none = _arch_b(accumulate=1), _arch_b(accumulate=None)
    assert one.optimizer.acc is None and none.optimizer.acc is None and one.accumulate == none.accumulate == 1
    for x, y in _batches(2):
        la, _ = one.train_step(x, y)
        lb, _ = none.train_step(x, y)
        assert la.item() == lb.item() and one.pending_micro_steps == 0
    _assert_same_state(_state(one), _state(none), "accumulate=1 against accumulate=None")
    assert _state(one)["step"] == 2
    one.flush_step()                                                    # nothing is ever pending
    _assert_same_state(_state(one), _state(none), "flush_step with accumulate=1")


def test_captured_replay_equals_eager_over_two_groups():
    eager, graph = _arch_b(accumulate=3), _arch_b(accumulate=3)
    bs = _batches(6)
    graph.capture_graph(*bs[0])
    _assert_same_state(_state(eager), _state(graph), "capture must not change the training state")
    assert graph.pending_micro_steps == 0 and _all_plus_zero(graph.optimizer.acc) and graph._graph_micro is not None
    for i, (x, y) in enumerate(bs):
        l0, p0 = eager.train_step(x, y)
        l1, p1 = graph.train_step(x, y)
        torch.cuda.synchronize()
        assert l0.item() == l1.item() and torch.equal(p0, p1), f"step {i}: the replay returns the micro-batch's loss and probabilities"
        assert eager.pending_micro_steps == graph.pending_micro_steps == (i + 1) % 3
        _assert_same_state(_state(eager), _state(graph), f"step {i}")
        assert torch.equal(eager.optimizer.acc.view(torch.int32), graph.optimizer.acc.view(torch.int32)), f"step {i}: accumulator"
        assert _state(graph)["step"] == (i + 1) // 3
    assert _all_plus_zero(graph.optimizer.acc)


def test_capture_inside_a_group_keeps_the_group():
    eager, graph = _arch_b(accumulate=2), _arch_b(accumulate=2)
    bs = _batches(2)
    eager.train_step(*bs[0])
    graph.train_step(*bs[0])
    graph.capture_graph(*bs[1])                                         # the warm-up's accumulator goes back to what the group holds
    assert graph.pending_micro_steps == 1
    assert torch.equal(eager.optimizer.acc.view(torch.int32), graph.optimizer.acc.view(torch.int32))
    eager.train_step(*bs[1])
    graph.train_step(*bs[1])
    _assert_same_state(_state(eager), _state(graph), "a group finished by the captured step")
    assert _state(graph)["step"] == 1


def test_flush_step_divides_a_short_group_by_n():
    net, twin = _arch_b(accumulate=3), _arch_b()
    (x, y), = _batches(1)
    net.flush_step()
    _assert_same_state(_state(net), _state(twin), "flush_step with nothing pending")
    g, _, _ = _twin_gradient(twin, x, y)
    net.train_step(x, y)
    assert net.pending_micro_steps == 1
    net.flush_step()
    assert net.pending_micro_steps == 0
    _twin_update(twin, [g, torch.zeros_like(g), torch.zeros_like(g)], 3)
    _assert_same_state(_state(net), _state(twin), "one micro-step of a group of 3, flushed")
    assert _state(net)["step"] == 1 and _all_plus_zero(net.optimizer.acc)
    net.flush_step()
    _assert_same_state(_state(net), _state(twin), "a second flush_step")


def test_ema_moves_once_per_group():
    avg = {"mode": "ema", "decay": 0.5}
    net, twin = _arch_b(accumulate=2, average=avg), _arch_b(average=avg)
    first = net.optimizer.avg.clone()
    assert torch.equal(first, net.flat.flat)
    grads = []
    for i, (x, y) in enumerate(_batches(4)):
        grads.append(_twin_gradient(twin, x, y)[0])
        before = net.optimizer.avg.clone()
        net.train_step(x, y)
        torch.cuda.synchronize()
        if i % 2 == 0:
            assert torch.equal(net.optimizer.avg, before), f"micro-step {i}: the average moved inside a group"
        else:
            _twin_update(twin, grads[-2:], 2)
            assert not torch.equal(net.optimizer.avg, before)
            assert torch.equal(net.optimizer.avg.view(torch.int32), twin.optimizer.avg.view(torch.int32)), f"group {i // 2}: the average"
            _assert_same_state(_state(net), _state(twin), f"group {i // 2}")
    assert net.optimizer.average_state() == ("ema", 2, 2)


def test_save_refuses_pending_micro_steps(tmp_path):
    net = _arch_b(accumulate=2)
    (x, y), = _batches(1)
    net.train_step(x, y)
    with pytest.raises(RuntimeError, match="flush_step"):
        net.save(str(tmp_path / "m.pt"))
    net.flush_step()
    net.save(str(tmp_path / "m.pt"))
    fresh = _arch_b(seed=9, accumulate=2)
    fresh.load(str(tmp_path / "m.pt"))
    _assert_same_state(_state(fresh), _state(net), "save / load after the flush")
    fresh.train_step(x, y)
    before = _state(fresh)
    with pytest.raises(RuntimeError, match="flush_step"):             # a load inside a group would mix the old weights' gradients into the new ones
        fresh.load(str(tmp_path / "m.pt"))
    _assert_same_state(_state(fresh), before, "a refused load")
    assert fresh.pending_micro_steps == 1


# ------------------------------------------------------------------------------------------------ data parallel, one GPU
@pytest.fixture(scope="module")
def rccl_world1():
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        port = 29900 + os.getpid() % 90
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)   # "nccl" is RCCL on ROCm
        created = True
    yield dist
    if created:
        dist.destroy_process_group()


def test_data_parallel_replicas_with_a_captured_step(rccl_world1):
    """tests/test_gpu_step.py's in-process RCCL group: two replicas with N = 2 in the data-parallel order (the accumulate launch, then the
    per-replica clip of the MEAN, the exchange, the already-clipped Adam), one eager and one replaying its three graphs (micro-step, finishing
    step, update); a plain accumulating model beside them.  One exchange per group; identical weights after two groups."""
    from ultrasound_modeling_amd.MainParallel import MirroredTrainer
    plain, a, b = _arch_b(seed=5, accumulate=2), _arch_b(seed=5, accumulate=2), _arch_b(seed=5, accumulate=2)
    exchanges = {}
    for name, net in (("a", a), ("b", b)):
        MirroredTrainer(net, force=True)
        inner = net.grad_sync
        assert inner is not None and getattr(inner, "chunks", None) is None

        class Counting:
            chunks = None

            def __init__(self, inner, name):
                self.inner, self.name = inner, name

            def __call__(self, g):
                exchanges[self.name] = exchanges.get(self.name, 0) + 1
                self.inner(g)
        net.grad_sync = Counting(inner, name)
    bs = _batches(4)
    b.capture_graph(*bs[0])
    assert b._graph_micro is not None and b._graph[1] is not None
    for i, (x, y) in enumerate(bs):
        lp, _ = plain.train_step(x, y)
        la, _ = a.train_step(x, y)
        lb, _ = b.train_step(x, y)
        torch.cuda.synchronize()
        assert lp.item() == la.item() == lb.item(), i
        assert exchanges.get("a", 0) == exchanges.get("b", 0) == (i + 1) // 2, "one exchange per optimiser step, none for a micro-step"
        _assert_same_state(_state(a), _state(b), f"step {i}: eager against replayed replica")
        _assert_same_state(_state(a), _state(plain), f"step {i}: data-parallel order against the plain step")
    assert _state(b)["step"] == 2 and torch.equal(a.flat.flat, b.flat.flat)
    gn = float(plain.optimizer.sumsq[0].item()) ** 0.5                                   # the norm of the last group's mean gradient
    assert abs(float(b.flat.grad.double().norm().item()) - min(gn, 1.0)) < 1e-3          # the exchanged buffer: the clipped mean


# ------------------------------------------------------------------------------------------------ the other three models
def _two_micro_steps(net, step, xs):
    start = _state(net)
    step(xs[0])
    assert net.pending_micro_steps == 1
    _assert_same_state(_state(net), start, "the first micro-step must not touch weights, moments or the step counter")
    assert net.optimizer.acc.abs().max().item() > 0
    step(xs[1])
    end = _state(net)
    assert net.pending_micro_steps == 0 and end["step"] == 1 and not torch.equal(end["p"], start["p"]) and _all_plus_zero(net.optimizer.acc)
    assert torch.isfinite(end["p"]).all()


def test_transunet_variant_accumulates():
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer
    net = VisionTransformer(img_size=(64, 128), batch_size=2, in_channels=1, accumulate=2)        # tests/test_gpu_transunet.py's smallest
    _two_micro_steps(net, lambda b: net.step(b[0], b[1], train=True), _batches(2, W=128))


def test_arch_a_accumulates_with_fresh_dropout_masks_per_micro_step():
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    net = ResNest(64, 64, 1, 3, ksize=3, radix=3, kpaths=4, learning_rate=5e-3, accumulate=2)
    masks = []

    def step(b):
        net.step(b[0], b[1], train=True)
        masks.append([m.clone() for m in net.resModel._masks if m is not None])
    _two_micro_steps(net, step, _batches(2))
    assert len(masks[0]) == 3
    for m0, m1 in zip(*masks):                                          # the step counter stood still between them; the masks did not
        assert ((m0 > 0) != (m1 > 0)).float().mean().item() > 0.4


def test_arch_a_resumes_its_mask_count_from_a_checkpoint(tmp_path):
    """The masks follow a count of the micro-steps, which a checkpoint does not hold: a load sets it to step * N, what it was at the save
    (checkpoints are written between groups), so the resumed run draws the masks the uninterrupted run draws."""
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    kw = dict(ksize=3, radix=3, kpaths=4, learning_rate=5e-3, accumulate=2)
    run, resumed = ResNest(64, 64, 1, 3, **kw), ResNest(64, 64, 1, 3, **kw)
    bs = _batches(3)
    for b in bs[:2]:
        run.step(b[0], b[1], train=True)
    path = run.save_params(str(tmp_path / "a.pt"))
    resumed.load_params_file(path)
    assert int(run._micro_dev.item()) == int(resumed._micro_dev.item()) == 2 and int(resumed.optimizer.step_dev.item()) == 1
    run.step(bs[2][0], bs[2][1], train=True)
    resumed.step(bs[2][0], bs[2][1], train=True)
    torch.cuda.synchronize()
    m_run, m_res = ([m for m in n.resModel._masks if m is not None] for n in (run, resumed))
    assert len(m_run) == 3 and all(torch.equal(a, b) for a, b in zip(m_run, m_res))
    assert torch.equal(run.optimizer.acc.view(torch.int32), resumed.optimizer.acc.view(torch.int32))


def test_swin_encoder_accumulates():
    from ultrasound_modeling_amd.SwinTransformer import SwinTransformerModel
    net = SwinTransformerModel(model_name="t", img_size=(64, 64), patch_size=(4, 4), in_chans=1, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                               window_size=8, seed=3, accumulate=2)
    g = torch.Generator().manual_seed(11)
    xs = [(torch.randn(2, 64, 64, 1, generator=g), torch.randn(2, 192, generator=g)) for _ in range(2)]
    _two_micro_steps(net, lambda b: net.train_step(b[0], b[1]), xs)
