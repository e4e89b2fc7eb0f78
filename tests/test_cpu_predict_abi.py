"""The inference entry points of the fused stem and cardinal kernels (usseg_stem_fwd_infer, usseg_cardinal_fwd_infer) and the predict
counter (usseg_counter_add) reject bad arguments with the library's error code and message before anything is launched, and
PredictDriver replays its captured graph only for an input of the captured shape, dtype and strides."""
import ctypes as C

import pytest
import torch

from ultrasound_modeling_amd.step import PredictDriver


def _lib():
    from ultrasound_modeling_amd import _lib as L
    return L, L.load()


def _stem_args(**kw):
    a = dict(B=1, H=16, W=16, x=16, ldx=8, w1=16, b1=16, w2=16, b2=16, w3=16, b3=16, gamma=16, beta=16, mean=16, var=16, eps=1e-3,
             alpha=0.3, pooled=16, stream=None)
    a.update(kw)
    return list(a.values())


def test_stem_fwd_infer_rejects_null_pointers():
    _, lib = _lib()
    for name in ("x", "w1", "b3", "var", "pooled"):
        assert lib.usseg_stem_fwd_infer(*_stem_args(**{name: None})) == -1, name
        assert b"stem_fwd_infer: null pointer" in lib.usseg_last_error()


@pytest.mark.parametrize("bad", [dict(H=15), dict(W=7), dict(B=0), dict(ldx=4), dict(ldx=12)])
def test_stem_fwd_infer_rejects_bad_geometry(bad):
    _, lib = _lib()
    assert lib.usseg_stem_fwd_infer(*_stem_args(**bad)) == -1
    assert b"stem_fwd_infer: bad geometry" in lib.usseg_last_error()


def test_stem_fwd_infer_rejects_misaligned_vectors():
    _, lib = _lib()
    assert lib.usseg_stem_fwd_infer(*_stem_args(gamma=20)) == -1
    assert b"16-byte aligned" in lib.usseg_last_error()


def _card(L, **kw):
    a = dict(B=1, H=8, W=8, Cin=32, P=3, cv11=3, cvkk=10, Up=16, Vp=32, Oc=64, ldx=32, ldu=16, ldv=32, ldsc=64, eps=1e-3, alpha=0.3)
    a.update(kw)
    return L.CardinalDesc(*a.values())


def test_cardinal_fwd_infer_rejects_unsupported_configurations():
    L, lib = _lib()
    for bad in (dict(Cin=48, ldx=48), dict(P=2), dict(cvkk=11), dict(Up=24), dict(Oc=96, ldsc=96)):
        d = _card(L, **bad)
        assert lib.usseg_cardinal_supported(C.byref(d)) == 0
        assert lib.usseg_cardinal_fwd_infer(C.byref(d), *([16] * 17)) == -1, bad
        assert b"cardinal_fwd_infer: no fused kernel" in lib.usseg_last_error()
    assert lib.usseg_cardinal_fwd_infer(None, *([16] * 17)) == -1


def test_cardinal_fwd_infer_rejects_null_pointers_and_bad_strides():
    L, lib = _lib()
    d = _card(L)
    assert lib.usseg_cardinal_supported(C.byref(d)) == 1
    for i in range(16):                 # every pointer argument but the stream
        args = [16] * 17
        args[i] = None
        assert lib.usseg_cardinal_fwd_infer(C.byref(d), *args) == -1, i
        assert b"cardinal_fwd_infer: null pointer" in lib.usseg_last_error()
    for bad in (dict(ldv=24), dict(ldsc=56), dict(ldx=24), dict(ldx=36), dict(B=0)):
        assert lib.usseg_cardinal_fwd_infer(C.byref(_card(L, **bad)), *([16] * 17)) == -1, bad
        assert b"cardinal_fwd_infer: bad geometry" in lib.usseg_last_error()
    args = [16] * 17
    args[2] = 20                        # b1 misaligned
    assert lib.usseg_cardinal_fwd_infer(C.byref(d), *args) == -1
    assert b"bias vectors must be 16-byte aligned" in lib.usseg_last_error()


def test_counter_add_rejects_a_null_counter():
    _, lib = _lib()
    assert lib.usseg_counter_add(None, 1, None) == -1
    assert b"counter_add: null pointer" in lib.usseg_last_error()


class _FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class _Driver(PredictDriver):
    """PredictDriver with a stand-in graph: only the host-side choice between replay and the eager body is exercised."""

    def __init__(self, x):
        self._px, self._pgraph, self._pprobs, self.eager = x.clone(), _FakeGraph(), torch.full((1,), 7.0), 0

    def _prep_x(self, x):
        return x

    def _predict_body(self, x):
        self.eager += 1
        return x.sum().reshape(1)


def test_predict_replays_only_for_the_captured_layout():
    d = _Driver(torch.zeros(4, 8, 6, 2))
    x = torch.arange(4 * 8 * 6 * 2, dtype=torch.float32).reshape(4, 8, 6, 2)
    assert d.predict(x) is d._pprobs and d._pgraph.replays == 1 and torch.equal(d._px, x)      # copied into the static buffer
    assert d.predict(d.predict_inputs()) is d._pprobs and d._pgraph.replays == 2
    # same first element, other shape / strides / dtype: eager, never the static buffer
    for other in (d._px[:1], d._px.transpose(1, 2).contiguous().transpose(1, 2), d._px.double(), d._px[..., :1]):
        before = d._px.clone()
        out = d.predict(other)
        assert out is not d._pprobs and d._pgraph.replays == 2
        assert torch.equal(d._px, before)
    assert d.eager == 4
