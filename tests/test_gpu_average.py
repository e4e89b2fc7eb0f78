"""GPU tests of the EMA / SWA weight averaging kept inside the optimiser step (csrc/average.hip).

Sizes: 1, 3, 4, 5 (scalar tail only / one float4 with and without a tail), 1023 and 1025 (around one workgroup of float4s), and
4*256*4096 + 4*256 + 3 - the smallest n at which the 4096-workgroup grid takes a second grid-stride trip and still has a scalar tail.

Per element the kernel must be within 2^-23 * (|p| + |avg_old|) of the fp64 restatement (tests/average_restatement.py: one rounding of
the difference plus one of the fused multiply-add); c == 0 must keep the bits of avg and c == 1 must store p itself.  Everything else is
BITWISE: the fused launch against ``adamw_step`` followed by ``average_update``, chunked against whole, eager against HIP-graph replay,
the averaged predict against a model loaded from ``save_averaged``, save / load against the uninterrupted run."""
import numpy as np
import pytest
import torch

import average_restatement as A
import usseg_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 4 * 256 * 4096 + 4 * 256 + 3
NS = [1, 3, 4, 5, 1023, 1025, BIG]
EMA = {"mode": "ema", "decay": 0.9, "dynamic_decay": True, "start_step": 4}
SWA = {"mode": "swa", "start": 5, "period": 3}


def _desc(cfg):
    from ultrasound_modeling_amd import flat
    return torch.from_numpy(flat._average_words(flat.average_config(cfg))).to(DEV)


def _coeff(cfg, t):
    if cfg["mode"] == "ema":
        return A.coeff(A.EMA, t, decay=cfg.get("decay", 0.999), dynamic_decay=cfg.get("dynamic_decay", False), start=cfg.get("start_step", 0))
    return A.coeff(A.SWA, t, start=cfg["start"], period=cfg["period"])


def _rand(n, seed, positive=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(n, generator=g, device=DEV, dtype=torch.float32)
    return t.abs() if positive else t


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_update(avg_new, avg_old, p, c, what):
    """One update of the device against the restatement: the bound, and the two bitwise cases."""
    an, ao, pn = avg_new.cpu().numpy(), avg_old.cpu().numpy(), p.cpu().numpy()
    if c == 0:
        assert np.array_equal(an.view(np.int32), ao.view(np.int32)), f"{what}: c == 0 must keep the bits of avg"
    elif c == 1:
        assert np.array_equal(an.view(np.int32), pn.view(np.int32)), f"{what}: c == 1 must store p itself"
    else:
        err = np.abs(an.astype(np.float64) - A.update64(ao, pn, c))
        bound = A.bound(ao, pn)
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), f"{what}: element {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e} (c = {c})"


# ------------------------------------------------------------------------------------------------ the kernels
# (settings, t): every branch of the coefficient - EMA before / at / after start, fixed and dynamic decay on either side of their crossing,
# SWA before start, its first (c = 1) and later snapshots, a step between snapshots, and mode off
CASES = [({"mode": "ema", "decay": 0.999}, 1), ({"mode": "ema", "decay": 0.9, "start_step": 4}, 4), ({"mode": "ema", "decay": 0.9, "start_step": 4}, 5),
         (EMA, 3), (EMA, 7), (EMA, 200), ({"mode": "ema", "decay": 0.0}, 2),
         (SWA, 4), (SWA, 5), (SWA, 8), (SWA, 9), (SWA, 35), ({"mode": "swa", "start": 0, "period": 1}, 2), (None, 3)]


@pytest.mark.parametrize("n", NS)
def test_average_update_against_the_restatement(n):
    from ultrasound_modeling_amd import ops
    p, avg0 = _rand(n, 1), _rand(n, 2)
    avg0[0] = -0.0                                                   # bits that an arithmetic pass would not keep
    if n > 4:
        _bits(avg0)[4] = 0x7FC12345                                  # a NaN with a payload (kept only if c == 0 moves no byte)
    for cfg, t in CASES:
        desc = torch.zeros(5, dtype=torch.int32, device=DEV) if cfg is None else _desc(cfg)
        c = np.float32(0) if cfg is None else _coeff(cfg, t)
        step = torch.full((1,), t, dtype=torch.int32, device=DEV)
        avg = avg0.clone()
        if c != 0 and c != 1 and n > 4:
            avg[4] = 0.5
        old = avg.clone()
        ops.average_update(avg, p, step, desc)
        _check_update(avg, old, p, c, f"n={n} {cfg} t={t}")
    assert {float(_coeff(c, t)) for c, t in CASES[:-1]} >= {0.0, 1.0}


@pytest.mark.parametrize("n", NS)
def test_fused_step_equals_adamw_step_then_average_update(n):
    from ultrasound_modeling_amd import ops
    p0, g, m0, v0, a0 = _rand(n, 3), _rand(n, 4) * 3.0, _rand(n, 5) * 0.1, _rand(n, 6, positive=True) * 0.01, _rand(n, 7)
    mask = (torch.arange(n, device=DEV) % 3 != 0).to(torch.uint8)
    sumsq = torch.zeros(ops.ACC_FLOATS, dtype=torch.float32, device=DEV)
    ops.sumsq(g, sumsq)
    assert n < 5 or float(sumsq[0].item()) > 1.0, "the clip must be active"
    lr_t = torch.full((1,), 3e-3, dtype=torch.float32, device=DEV)
    wd, wd0 = torch.full((1,), 0.01, dtype=torch.float32, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV)
    hyper = (0.9, 0.999, 1e-7)
    for cfg, t in ((EMA, 9), (SWA, 11), (SWA, 5), (SWA, 6)):
        desc, step = _desc(cfg), torch.full((1,), t, dtype=torch.int32, device=DEV)
        for use_mask in (False, True):
            for clip in (0.0, 1.0):
                for wd_t in (None, wd):
                    what = f"n={n} {cfg['mode']} t={t} mask={use_mask} clip={clip} wd={'null' if wd_t is None else 'on'}"
                    k = mask if use_mask else None
                    p1, m1, v1, a1 = p0.clone(), m0.clone(), v0.clone(), a0.clone()
                    ops.adamw_step(p1, g, m1, v1, sumsq, clip, lr_t, wd0 if wd_t is None else wd_t, k, *hyper)
                    ops.average_update(a1, p1, step, desc)
                    p2, m2, v2, a2 = p0.clone(), m0.clone(), v0.clone(), a0.clone()
                    ops.adamw_avg_step(p2, g, m2, v2, a2, sumsq, clip, lr_t, wd_t, k, *hyper, step, desc)
                    for name, x, y in (("p", p1, p2), ("m", m1, m2), ("v", v1, v2), ("avg", a1, a2)):
                        assert _same_bits(x, y), f"{what}: {name} differs in {(_bits(x) != _bits(y)).sum().item()} of {n} elements"
                    if wd_t is None:                      # no decay: the fixed-rate kernel's bits too
                        p3, m3, v3 = p0.clone(), m0.clone(), v0.clone()
                        ops.adam_clip_step(p3, g, m3, v3, sumsq, clip, lr_t, *hyper)
                        assert _same_bits(p3, p2) and _same_bits(m3, m2) and _same_bits(v3, v2), f"{what}: not adam_clip_step's bits"
                    else:
                        assert not torch.equal(p2, p0)
                    assert _same_bits(a2, a0) == (_coeff(cfg, t) == 0), what


@pytest.mark.parametrize("n", NS)
def test_swap_exchanges_and_twice_is_the_identity(n):
    from ultrasound_modeling_amd import ops
    a0, b0 = _rand(n, 8), _rand(n, 9)
    _bits(a0)[0] = 0x7FC00001
    a, b = a0.clone(), b0.clone()
    ops.swap_f32(a, b)
    assert _same_bits(a, b0) and _same_bits(b, a0)
    ops.swap_f32(a, b)
    assert _same_bits(a, a0) and _same_bits(b, b0)


# ------------------------------------------------------------------------------------------------ the optimiser
class _Flat:
    """What ``AdamClip`` needs of ``FlatParams``, at any n (``FlatParams`` pads to a multiple of 8: no scalar tail)."""

    def __init__(self, n, seed=10):
        self.device, self.total = torch.device(DEV), n
        self.flat = _rand(n, seed)
        self.grad = torch.zeros(n, dtype=torch.float32, device=DEV)
        self.names, self.params, self.offsets = [], [], []


def _opt(n, **kw):
    from ultrasound_modeling_amd.flat import AdamClip
    return AdamClip(_Flat(n), lr=kw.pop("lr", 1e-2), **kw)


def _opt_state(o):
    torch.cuda.synchronize()
    return dict(p=o.flat.flat.clone(), m=o.m.clone(), v=o.v.clone(), step=int(o.step_dev.item()), avg=None if o.avg is None else o.avg.clone())


@pytest.mark.parametrize("clip", [1.0, None])
def test_fixed_rate_optimiser_keeps_its_bits_with_an_average(clip):
    plain, avg = _opt(1029, clip_norm=clip), _opt(1029, clip_norm=clip, average={"mode": "ema", "decay": 0.9})
    assert not plain.scheduled and not avg.scheduled and avg.wd_t_dev is None
    for i in range(5):
        g = _rand(1029, 20 + i) * 2.0
        for o in (plain, avg):
            o.flat.grad.copy_(g)
            o.apply()
        a, b = _opt_state(plain), _opt_state(avg)
        assert a["step"] == b["step"] == i + 1
        for k in ("p", "m", "v"):
            assert _same_bits(a[k], b[k]), f"step {i}: {k}"
    assert not torch.equal(b["avg"], b["p"])


@pytest.mark.parametrize("cfg", [SWA, EMA], ids=["swa", "ema"])
def test_25_optimiser_steps_against_the_restatement(cfg):
    n = 1029
    o = _opt(n, clip_norm=1.0, average=cfg, weight_decay=0.01 if cfg is EMA else None)       # the table path and the fixed-rate path
    assert torch.equal(o.avg, o.flat.flat), "the average starts as a copy of the weights"
    snaps, slack = [], np.zeros(n)
    for i in range(25):
        t = i + 1
        old = o.avg.clone()
        o.flat.grad.copy_(_rand(n, 100 + i))
        o.apply()
        torch.cuda.synchronize()
        c = _coeff(cfg, t)
        _check_update(o.avg, old, o.flat.flat, c, f"{cfg['mode']} step {t}")
        if cfg is SWA and c != 0:
            snaps.append(o.flat.flat.double().cpu().numpy())
            # the step's own bound, plus the fp32 rounding of c = 1/k (at most 2^-25 for c <= 1/2) times |p - avg| <= |p| + |avg|
            slack += 1.25 * A.bound(old.cpu().numpy(), o.flat.flat.cpu().numpy())
    mode, t, k = o.average_state()
    assert (mode, t) == (cfg["mode"], 25)
    if cfg is SWA:          # t = 5, 8, ..., 23: the mean of 7 snapshots, up to the summed per-step bounds (a later blend only shrinks an earlier error)
        assert k == len(snaps) == 7
        assert np.all(np.abs(o.avg.double().cpu().numpy() - np.mean(snaps, axis=0)) <= slack)
    else:
        assert k == 21


@pytest.mark.parametrize("table", [False, True], ids=["fixed_rate", "table"])
def test_chunked_update_equals_one_launch(table):
    from ultrasound_modeling_amd.step import even_chunks
    n = 5 * 1024 + 517
    kw = dict(clip_norm=None, average={"mode": "ema", "decay": 0.75}, weight_decay=0.02 if table else None)
    whole, parts = _opt(n, **kw), _opt(n, **kw)
    ranges = even_chunks(n, 3)
    assert len(ranges) == 3 and ranges[-1][1] == n
    for i in range(2):
        g = _rand(n, 200 + i)
        for o in (whole, parts):
            o.flat.grad.copy_(g)
            o.advance()
        whole.apply_range(0, n)
        for lo, hi in ranges:
            parts.apply_range(lo, hi)
    a, b = _opt_state(whole), _opt_state(parts)
    assert a["step"] == b["step"] == 2
    for k in ("p", "m", "v", "avg"):
        assert _same_bits(a[k], b[k]), k
    assert not torch.equal(a["avg"], a["p"])


# ------------------------------------------------------------------------------------------------ the models
def _batches(n, B=2, H=64, W=64):
    return [tuple(t for t in O.synthetic_batch(B, H, W, 1, seed=40 + i)) for i in range(n)]


_PARAMS = {}


def _arch_b(average, seed=3):
    """The smallest Arch B of tests/test_gpu_step.py."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    if seed not in _PARAMS:
        _PARAMS[seed] = {k: v.float().double() for k, v in O.init_vision_transformer_params(channel=1, seed=seed, perturb=True).items()}
    net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1, learning_rate=1e-3, average=average)
    net.load_params(_PARAMS[seed])
    return net


def _state(net):
    torch.cuda.synchronize()
    return _opt_state(net.optimizer)


def _assert_same(a, b, what):
    assert a["step"] == b["step"], what
    for k in ("p", "m", "v", "avg"):
        assert (a[k] is None and b[k] is None) or _same_bits(a[k], b[k]), f"{what}: {k}"


def test_model_graph_replay_equals_eager_and_follows_a_new_decay():
    cfg = {"mode": "ema", "decay": 0.9}
    eager, graph = _arch_b(cfg), _arch_b(cfg)
    assert torch.equal(eager.optimizer.avg, eager.flat.flat), "load_params before the first step refreshes the average"
    bs = _batches(3)
    before = _state(graph)
    graph.capture_graph(bs[0][0], bs[0][1].float())
    _assert_same(before, _state(graph), "capture_graph must leave the average and the counter")
    assert before["step"] == 0
    for i in range(6):
        x, y = bs[i % 3]
        eager.train_step(x, y.float())
        graph.train_step(x, y.float())
        _assert_same(_state(eager), _state(graph), f"step {i}")
    assert graph._graph is not None and _state(graph)["step"] == 6 and not torch.equal(graph.optimizer.avg, graph.flat.flat)
    for net in (eager, graph):
        net.optimizer.set_average_decay(0.5)                      # no recapture
    old = graph.optimizer.avg.clone()
    eager.train_step(bs[0][0], bs[0][1].float())
    graph.train_step(bs[0][0], bs[0][1].float())
    _assert_same(_state(eager), _state(graph), "after set_average_decay")
    _check_update(graph.optimizer.avg, old, graph.flat.flat, np.float32(0.5), "the replay after set_average_decay(0.5)")
    assert graph.optimizer.average_state() == ("ema", 7, 7)


def test_averaged_weights_predict_and_leave(tmp_path):
    cfg = {"mode": "ema", "decay": 0.5}
    net, twin = _arch_b(cfg), _arch_b(cfg)
    bs = _batches(4)
    for x, y in bs[:3]:
        net.train_step(x, y.float())
        twin.train_step(x, y.float())
    x = bs[3][0]
    path = str(tmp_path / "avg.pt")
    net.save_averaged(path)
    assert not any(k.startswith("__adam_") for k in torch.load(path, map_location="cpu", weights_only=True))
    fresh = _arch_b(None)
    fresh.load(path)
    assert _same_bits(fresh.flat.flat, net.optimizer.avg) and not torch.equal(fresh.flat.flat, net.flat.flat)
    want = fresh.predict(x).clone()
    before, raw = _state(net), net.predict(x).clone()
    assert not torch.equal(raw, want)
    net.capture_predict_graph(x)
    assert _same_bits(net.predict(x), raw)
    with net.averaged_weights():
        assert net._pgraph is not None and _same_bits(net.predict(x), want), "captured predict graph inside averaged_weights()"
        assert _same_bits(net.predict(x[:1]), fresh.predict(x[:1])), "eager predict (another shape) inside averaged_weights()"
        assert _same_bits(net._predict_body(net._prep_x(x)), want), "eager predict inside averaged_weights()"
        with pytest.raises(RuntimeError):
            net.train_step(bs[0][0], bs[0][1].float())
        with pytest.raises(RuntimeError):
            with net.averaged_weights():
                pass
    _assert_same(before, _state(net), "leaving averaged_weights() restores the weights and the average")
    assert _same_bits(net.predict(x), raw), "and the packed operands"
    net.train_step(bs[3][0], bs[3][1].float())
    twin.train_step(bs[3][0], bs[3][1].float())
    _assert_same(_state(twin), _state(net), "the next step equals a twin's that never entered the block")
    with pytest.raises(ValueError):
        fresh.averaged_weights().__enter__()


def test_save_load_continues_bitwise_and_plain_checkpoints_load(tmp_path):
    bs = _batches(4)
    run = _arch_b(SWA_EARLY)
    for x, y in bs[:2]:
        run.train_step(x, y.float())
    path = str(tmp_path / "ckpt.pt")
    run.save(path)
    resumed = _arch_b({"mode": "ema", "decay": 0.3}, seed=5)          # other weights and settings: the checkpoint replaces them
    resumed.load(path)
    _assert_same(_state(run), _state(resumed), "after load")
    assert resumed.optimizer.average == run.optimizer.average
    for x, y in bs[2:]:
        run.train_step(x, y.float())
        resumed.train_step(x, y.float())
    _assert_same(_state(run), _state(resumed), "two steps after load")
    assert run.optimizer.average_state() == ("swa", 4, 3) and not torch.equal(run.optimizer.avg, run.flat.flat)
    plain = _arch_b(None)
    plain.train_step(bs[0][0], bs[0][1].float())
    ppath = str(tmp_path / "plain.pt")
    plain.save(ppath)
    assert "__adam_avg__" not in torch.load(ppath, map_location="cpu", weights_only=True)
    resumed.load(ppath)
    s = _state(resumed)
    assert s["step"] == 1 and _same_bits(s["p"], plain.flat.flat) and _same_bits(s["avg"], s["p"]), "the average starts from the loaded weights"


SWA_EARLY = {"mode": "swa", "start": 2, "period": 1}


def _changed_only_where_the_weights_did(net, p0, cfg):
    torch.cuda.synchronize()
    p, avg = net.flat.flat, net.optimizer.avg
    moved = _bits(p) != _bits(p0)
    assert moved.any() and not moved.all()                              # (padding between the variables never moves)
    assert _same_bits(avg[~moved], p0[~moved]), "avg changed where the weights did not"
    _check_update(avg, p0, p, _coeff(cfg, 1), "one step")
    assert (_bits(avg) != _bits(p0))[moved].float().mean().item() > 0.9


def test_arch_a_and_swin_steps_run_with_an_average():
    from ultrasound_modeling_amd.SwinTransformer import SwinTransformerModel
    from ultrasound_modeling_amd.TBI_ResNest import ResNest
    cfg = {"mode": "ema", "decay": 0.25}
    a = ResNest(64, 64, 1, 3, ksize=3, radix=3, kpaths=4, learning_rate=5e-3, average=cfg)
    P = {k: v.float().double() for k, v in O.init_archA_params(channel=1, radix=3, kpaths=4, seed=4, perturb=True).items()}
    a.load_params(P)
    p0 = a.flat.flat.clone()
    assert _same_bits(a.optimizer.avg, p0)
    x, y = _batches(1)[0]
    a.step(x, y.float(), train=True)
    _changed_only_where_the_weights_did(a, p0, cfg)
    s = SwinTransformerModel(model_name="t", img_size=(64, 64), patch_size=(4, 4), in_chans=1, embed_dim=96, depths=[2, 2], num_heads=[3, 6],
                             window_size=8, seed=3, average=cfg)
    p0 = s.flat.flat.clone()
    g = torch.Generator().manual_seed(11)
    s.train_step(torch.randn(2, 64, 64, 1, generator=g), torch.randn(2, 192, generator=g))
    _changed_only_where_the_weights_did(s, p0, cfg)


# ------------------------------------------------------------------------------------------------ data parallel, one GPU
@pytest.fixture(scope="module")
def rccl_world1():
    import os
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        port = 29600 + os.getpid() % 300
        dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)   # "nccl" is RCCL on ROCm
        created = True
    yield dist
    if created:
        dist.destroy_process_group()


def test_mirrored_chunked_step_keeps_the_same_average(rccl_world1):
    """``MirroredTrainer``'s chunk-pipelined update goes through ``apply_range``: the single-replica bits, the average included."""
    from ultrasound_modeling_amd.MainParallel import MirroredTrainer
    cfg = {"mode": "ema", "decay": 0.9}
    plain, dp = _arch_b(cfg, seed=5), _arch_b(cfg, seed=5)
    tr = MirroredTrainer(dp, force=True, chunks=3)
    assert getattr(dp.grad_sync, "chunks", None) is not None
    for i, (x, y) in enumerate(_batches(2)):
        plain.train_step(x, y.float())
        tr.train_step(x, y.float())
        _assert_same(_state(plain), _state(dp), f"chunked step {i}")
    assert not torch.equal(dp.optimizer.avg, dp.flat.flat)


# ------------------------------------------------------------------------------------------------ the drivers
def test_mainnumpy_main_validates_and_saves_the_averaged_model(tmp_path, monkeypatch, capsys):
    import math
    from test_gpu_metrics import _raw
    from ultrasound_modeling_amd import MainNumpy
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    np.save(tmp_path / "train.npy", _raw(4, 64, 64, 10, seed=1))
    np.save(tmp_path / "val.npy", _raw(2, 64, 64, 10, seed=2))
    monkeypatch.setattr(MainNumpy, "input_size", (64, 64))
    path = str(tmp_path / "m.pt")
    net, proc = MainNumpy.main(str(tmp_path / "train.npy"), str(tmp_path / "val.npy"), path, epochs=5, batch_size=2, average="ema:0.5")
    out = capsys.readouterr().out
    test = [h for h in proc.history if h["phase"] == "test"]
    assert len(test) == 1 and "loss (raw weights) = " in out                           # epoch 5 tests
    assert math.isfinite(test[0]["loss"]) and math.isfinite(test[0]["raw_loss"]) and test[0]["loss"] != test[0]["raw_loss"]
    assert net.optimizer.average_state() == ("ema", 10, 10) and not net._averaged
    raw, avg = VisionTransformer(2, img_size=(64, 64)), VisionTransformer(2, img_size=(64, 64))
    raw.load(path)
    avg.load(path + ".avg")
    assert _same_bits(raw.flat.flat, net.flat.flat) and _same_bits(avg.flat.flat, net.optimizer.avg)
    x, y, _ = _val_batch(tmp_path)
    with net.averaged_weights():
        want = net.step(x, y)[0].item()
    assert avg.step(x, y)[0].item() == want != raw.step(x, y)[0].item()


def _val_batch(tmp_path):
    from ultrasound_modeling_amd.Dataset_2 import Dataset
    return Dataset(str(tmp_path / "train.npy"), str(tmp_path / "val.npy"), 3).next_test(16)
