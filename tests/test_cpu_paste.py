"""The lesion copy-paste without a GPU: the option string, the host draws and their independence of ``DataAugs.draw`` and of the warp, the bank
restatement against the hand-stated fixture, the conditions that keep the device comparison (tests/test_gpu_paste.py) from passing vacuously -
asserted on the NumPy restatement (tests/paste_restatement.py) alone - two closed forms of the restatement, the structs against the header
text, the symbol, and every argument check of csrc/paste.hip (an error code and a message before any launch)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import paste_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HostBank(object):
    """What ``draw_paste`` reads of a ``LesionBank``: the table."""
    def __init__(self, table):
        self.table = table


# ------------------------------------------------------------------------------------------------ the option string
def test_parse_paste_round_trip_and_refusals():
    from ultrasound_modeling_amd import paste as Pp
    d = Pp.parse_paste("p=0.5,max_lesions=2,min_area=4,min_landed=0.5,flip=1,shift=none,protect=1,connectivity=8")
    assert d == {"p": 0.5, "max_lesions": 2, "min_area": 4, "min_landed": 0.5, "flip": True, "shift": None, "protect": True, "connectivity": 8}
    assert d == Pp.parse_paste("") == Pp.paste_config() == Pp.paste_config(None)
    c = Pp.parse_paste(" shift=3:2, p=1 ,max_lesions=4,flip=false,protect=0 , connectivity=4,min_area=1,min_landed=0.25")
    assert c == {"p": 1.0, "max_lesions": 4, "min_area": 1, "min_landed": 0.25, "flip": False, "shift": (3, 2), "protect": False, "connectivity": 4}
    assert Pp.parse_paste("shift=5")["shift"] == (5, 5) and Pp.paste_config({"shift": 0})["shift"] == (0, 0)
    for cfg in (c, d, Pp.paste_config({"shift": (0, 7)})):
        assert Pp.parse_paste(Pp.format_paste(cfg)) == cfg and Pp.paste_config(Pp.format_paste(cfg)) == cfg and Pp.paste_config(cfg) == cfg
    for bad in ("p=1.5", "p=-0.1", "p=nan", "max_lesions=0", "max_lesions=5", "max_lesions=1.5", "min_area=0", "min_area=-3", "min_area=2.5",
                "min_landed=1.5", "min_landed=-1", "min_landed=nan", "flip=2", "flip=maybe", "protect=", "shift=-1:0", "shift=1:2:3", "shift=a:b",
                "shift=1.5", "connectivity=6", "connectivity=8.5", "p", "p=", "p=1:2", "blend=3", "p=0.5,p=0.5", "max_lesions=inf"):
        with pytest.raises(ValueError, match="paste"):
            Pp.parse_paste(bad)
    for bad in ({"ps": 3}, {"p": "x"}, {"p": True}, {"shift": (1, 2, 3)}, {"shift": "x"}, {"flip": "yes"}, {"max_lesions": None}, {"connectivity": True}, 3, [1]):
        with pytest.raises(ValueError, match="paste"):
            Pp.paste_config(bad)
    with pytest.raises(ValueError):
        Pp.parse_paste(None)
    assert Pp.MAX_ITEMS == 4
    assert "NOBODY HAS" in Pp.__doc__ and "MEASURED" in Pp.__doc__          # the defaults are documented as unmeasured


# ------------------------------------------------------------------------------------------------ the draws
def _bank(H=12, W=9, min_area=1):
    return _HostBank(R.bank_of(R.layout(H, W), 8, min_area)[1])


def _target_box(it, W):
    r0, c0, r1, c1 = it["box"]
    f0, f1 = (W - 1 - c1, W - 1 - c0) if it["flip"] else (c0, c1)
    return r0 + it["dr"], f0 + it["dc"], r1 + it["dr"], f1 + it["dc"]


@pytest.mark.parametrize("shift", [None, (2, 1), (0, 0)], ids=str)
def test_draw_paste(shift):
    from ultrasound_modeling_amd import paste as Pp
    H, W = 24, 18
    bank = _bank(H, W)
    cfg = Pp.paste_config({"p": 0.5, "max_lesions": 3, "shift": shift, "min_landed": 0.3})
    a = [Pp.draw_paste(random.Random(3), cfg, bank, H, W) for _ in range(2)]
    assert a[0] == a[1]                                             # two generators with the same seed agree
    rng = random.Random(4)
    draws = [Pp.draw_paste(rng, cfg, bank, H, W) for _ in range(400)]
    assert 150 < sum(d["active"] for d in draws) < 250
    assert {d["n"] for d in draws} == {1, 2, 3} and all(len(d["items"]) == 3 for d in draws)
    flips, moved, seen = 0, 0, set()
    for d in draws:
        for it in d["items"]:
            row = next(t for t in bank.table if t[0] == it["record"] and t[1] == it["comp"])
            assert it["box"] == tuple(row[3:]) and it["area"] == row[2] and it["need"] == max(1, int(np.ceil(0.3 * row[2])))
            t = _target_box(it, W)
            assert 0 <= t[0] <= t[2] < H and 0 <= t[1] <= t[3] < W, (it, t)            # the box stays inside the image
            if shift is not None:
                assert abs(it["dr"]) <= shift[0] and abs(it["dc"]) <= shift[1]
            flips += it["flip"]
            moved += it["dr"] != 0 or it["dc"] != 0
            seen.add((it["record"], it["comp"]))
    assert seen == {(0, 1), (0, 2), (1, 1)}                         # uniform over the bank: every lesion is drawn
    assert 450 < flips < 750                                        # 1200 coins
    assert (moved == 0) if shift == (0, 0) else moved > 600
    assert not any(it["flip"] for _ in range(50) for it in Pp.draw_paste(rng, dict(cfg, flip=False), bank, H, W)["items"])
    assert not any(Pp.draw_paste(rng, dict(cfg, p=0.0), bank, H, W)["active"] for _ in range(200))
    assert all(Pp.draw_paste(rng, dict(cfg, p=1.0), bank, H, W)["active"] for _ in range(200))
    # the state after n draws does not depend on which samples were active, nor on whether lesions are flipped
    r0, r1, r2 = random.Random(8), random.Random(8), random.Random(8)
    for _ in range(5):
        Pp.draw_paste(r0, dict(cfg, p=0.0), bank, H, W), Pp.draw_paste(r1, dict(cfg, p=1.0), bank, H, W)
        Pp.draw_paste(r2, dict(cfg, p=1.0, flip=False), bank, H, W)
    assert r0.getstate() == r1.getstate()
    # (without flips other column ranges are drawn, so only the NUMBER of draws is the same: 2 + 4 * max_lesions calls each)
    calls = []

    class Counting(object):                                         # a proxy, not a subclass: the generator's own methods stay as they are
        def __init__(self, seed):
            self.rng = random.Random(seed)

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self.rng, name)
    per = []
    for kw in (dict(p=0.0), dict(p=1.0), dict(p=1.0, flip=False)):
        calls.clear()
        Pp.draw_paste(Counting(5), dict(cfg, **kw), bank, H, W)
        per.append([c for c in calls])
    assert per[0] == per[1] == per[2]
    assert per[0] == ["random", "randint"] + ["randrange", "random", "randint", "randint"] * 3      # active, the count; per slot lesion, coin, two shifts


def _recording_dataset(**kw):
    from ultrasound_modeling_amd.Dataset import Dataset

    class _Recording(Dataset):
        """The real iterator; the bank from the restatement and the launches (paste, warp, augment) replaced by a record of their arguments."""
        def __init__(self, **kw):
            self.order = []
            super().__init__(device="cpu", **kw)
            self.params, self.warps, self.pastes = [], [], []

        def _lesion_bank(self, cfg):
            from ultrasound_modeling_amd.paste import LesionBank
            labels, table = R.bank_of(self.y_tr.numpy(), cfg["connectivity"], cfg["min_area"])
            return LesionBank(labels=labels, table=table)

        def pasted(self, x, y, params):
            assert self.paste is not None and len(params) == x.shape[0]
            self.pastes.append(params)
            self.order.append("paste")
            return x, y

        def warped(self, x, y, warp_params):
            self.warps.append(warp_params)
            self.order.append("warp")
            return x, y

        def _augment(self, x, y, params):
            self.params.append(params)
            self.order.append("augment")
            return x.float(), y

        def _plain(self, x, y):
            return x.float(), y
    raw = np.random.default_rng(2).random((7, 1, 12, 9, 12))
    raw[:, 0, :, :, 0] = np.concatenate([R.layout(12, 9), R.layout(12, 9), R.layout(12, 9)[:1]])
    return _Recording(train_data=raw, val_data=raw[:2], batch_size=4, **kw)


def test_paste_draws_leave_the_other_draw_sequences_alone_and_the_replicas_agree():
    from ultrasound_modeling_amd import paste as Pp
    cfg, wcfg = {"p": 0.5, "min_area": 1}, {"sigma": 1.0, "p": 0.5}
    plain = _recording_dataset(warp=wcfg, warp_seed=21)
    assert plain.paste is None and plain.draw_pastes(3) is None and plain.paste_report() is None
    list(plain.train_batches(rng=random.Random(6)))
    whole = _recording_dataset(warp=wcfg, warp_seed=21, paste=cfg, paste_seed=33)
    assert len(whole.paste_bank) == 8 and whole.paste_bank.labels.shape == (7, 12, 9)
    list(whole.train_batches(rng=random.Random(6)))
    assert whole.params == plain.params and whole.warps == plain.warps        # neither generator is advanced by the paste
    assert whole.order == ["paste", "warp", "augment"] * 2                     # paste, then warp, then dataAug
    assert [len(p) for p in whole.pastes] == [4, 3]
    rp = random.Random(33)
    want = [Pp.draw_paste(rp, Pp.paste_config(cfg), whole.paste_bank, 12, 9) for _ in range(7)]
    assert whole.pastes[0] + whole.pastes[1] == want                           # the paste's own generator, in sample order
    assert whole.paste_drawn == sum(d["n"] for d in want if d["active"]) > 0
    ranks = [_recording_dataset(warp=wcfg, warp_seed=21, paste=cfg, paste_seed=33) for _ in range(2)]
    for r, ds in enumerate(ranks):
        list(ds.train_batches(r, 2, rng=random.Random(6)))
    assert ranks[0].pastes[0] + ranks[1].pastes[0] == want[:4] and ranks[0].pastes[1] + ranks[1].pastes[1] == want[4:]
    assert ranks[0].params[0] + ranks[1].params[0] == plain.params[0]
    list(whole.test_batches())                                                 # validation batches are never pasted
    assert [len(p) for p in whole.pastes] == [4, 3]


def test_the_drivers_take_the_option():
    import inspect
    from ultrasound_modeling_amd import Dataset, Dataset_2, MainNumpy, MainParallel, TBI_TransUNet
    for fn in (MainNumpy.main, MainParallel.main, TBI_TransUNet.main, Dataset_2.Dataset.__init__, Dataset.Dataset.__init__, TBI_TransUNet.Dataset.__init__):
        assert inspect.signature(fn).parameters["paste"].default is None, fn
    for fn in (Dataset_2.Dataset.__init__, Dataset.Dataset.__init__, TBI_TransUNet.Dataset.__init__, MainNumpy.main):
        assert inspect.signature(fn).parameters["paste_seed"].default == 0, fn
    for fn, before in ((MainNumpy.main, "accumulate"), (TBI_TransUNet.main, "accumulate"), (MainParallel.main, "accumulate"), (Dataset_2.Dataset.__init__, "warp_seed")):
        names = list(inspect.signature(fn).parameters)
        assert names.index("paste") > names.index(before), fn                 # new keyword arguments go at the end
    with pytest.raises(SystemExit, match="paste"):
        MainParallel._cli(["tr.npy", "va.npy", "--paste", "max_lesions=9"])    # refused before any rank starts
    raw = np.random.default_rng(2).random((3, 1, 6, 5, 12))
    with pytest.raises(ValueError, match="paste"):
        Dataset_2.Dataset(train_data=raw, val_data=raw, device="cpu", paste={"p": 2})
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # the bank is labelled on the device
        Dataset_2.Dataset(train_data=raw, val_data=raw, device="cpu", paste={})
    from ultrasound_modeling_amd.paste import LesionBank, paste_line
    with pytest.raises(ValueError, match="no lesion"):
        LesionBank(labels=np.zeros((2, 4, 4), np.int32), table=np.zeros((0, 7), np.int64))
    assert paste_line(3, 5, 40) == "paste: 3 of 5 lesions placed, 40 pixels pasted"


def test_the_drivers_print_one_line_per_report_and_nothing_without_paste(capsys):
    from ultrasound_modeling_amd import MainNumpy, MainParallel

    class _On(object):
        paste, reads = {"p": 1.0}, 0

        def paste_report(self):
            self.reads += 1
            return 3, 5, 40

    class _Off(object):
        paste = None

        def paste_report(self):
            return None
    on = _On()
    assert MainNumpy.paste_report(on) == (3, 5, 40) and MainParallel.Process(4)._paste_report(on) == (3, 5, 40) and on.reads == 2      # one read-back each
    assert capsys.readouterr().out == "paste: 3 of 5 lesions placed, 40 pixels pasted\n" * 2
    assert MainNumpy.paste_report(_Off()) is None and MainNumpy.paste_report(object()) is None
    assert MainParallel.Process(4)._paste_report(_Off()) is None and MainParallel.Process(4)._paste_report(object()) is None
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_bank_restatement_gives_the_hand_stated_lesions():
    labels, table = R.bank_of(R.layout(12, 9), 8, 1)
    assert table.tolist() == [[0, 1, 12, 2, 1, 4, 4], [0, 2, 1, 11, 8, 11, 8], [1, 1, 6, 1, 1, 4, 3]]
    assert [int(labels[n].max()) for n in range(3)] == [2, 1, 0]
    assert R.bank_of(R.layout(12, 9), 8, 4)[1][:, :3].tolist() == [[0, 1, 12], [1, 1, 6]]          # min_area drops the soft pixel
    assert (labels[0] == 1).sum() == 12 and labels[0, 11, 8] == 2 and (labels[1] == 1).sum() == 6 and not labels[2].any()
    y = R.layout(12, 9)
    assert y[1, 4, 1] == 2.0 and y[1, 4, 3] == np.float32(1.2) and y[0, 11, 8] == 1.5 and not y[:, 0].any() and not y[:, :, 0].any()
    d = np.zeros((1, 4, 4), np.float32)
    d[0, 0, 0] = d[0, 1, 1] = 2                                             # a diagonal pair: one lesion at connectivity 8, two at 4
    assert len(R.bank_of(d, 8)[1]) == 1 and len(R.bank_of(d, 4)[1]) == 2
    for H, W, _ in R.SHAPES:
        kr, kc = H // 12, max(1, W // 9)
        t = R.bank_of(R.layout(H, W), 8, 1)[1]
        assert t[:, :2].tolist() == [[0, 1], [0, 2], [1, 1]]
        assert t[:, 2].tolist() == [3 * kr * min(4 * kc, W - 1), 1, 4 * kr * kc + kr * 2 * kc]


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_the_cases_cannot_pass_vacuously(shape):
    on, off = R.decided(shape, 0, True), R.decided(shape, 0, False)
    for d in (on, off):
        assert d["counts"][0] >= 1 and d["rejected"] >= 1 and d["overwritten"] >= 1 and d["refused"] >= 1, {k: d[k] for k in ("counts", "rejected", "overwritten", "refused")}
    assert int((on["src"] != off["src"]).sum()) >= 1                            # at least one pixel changed by protect
    assert on["landed"][1, 0] < off["landed"][1, 0]                             # the recipient's own bleed
    t0, t1 = R.case(shape, np.float32)["tables"]
    assert on["landed"][0].tolist()[:2] == [t0[0]["items"][0]["area"], t0[0]["items"][1]["area"]]       # both land whole
    assert 0 < on["landed"][2, 0] < t0[2]["items"][0]["area"] and 0 < on["landed"][2, 1] < t0[2]["items"][1]["need"]
    assert not on["landed"][3, 1:].any() and not on["landed"][4:].any()         # items that do not exist, n_items = 0, the inactive sample
    assert (on["src"][4:] < 0).all() and (on["src"][3] >= 0).sum() == on["landed"][3, 0] == t0[3]["items"][0]["area"] - 1    # the NaN label
    alt = R.decided(shape, 1, True)
    assert alt["counts"][0] >= 4 and (alt["src"][0] < 0).all() and (alt["src"][2] < 0).all() and (alt["landed"][1] > 0).all()
    assert not np.array_equal(alt["src"], on["src"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_closed_forms_of_the_restatement(shape, dtype):
    c = R.case(shape, dtype)
    H, W, Cc = shape
    A, Lz = c["table"][0], c["table"][2]
    bits = lambda a: np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    # a lesion pasted in place into its own record changes nothing
    for rec, lesion in ((0, A), (1, Lz)):
        x, y = c["x_bank"][rec:rec + 1], c["y_bank"][rec:rec + 1]
        for protect in (False, True):
            xo, yo, landed, counts, _ = R.paste(x, y, [{"active": 1, "n": 1, "items": [R.item(lesion, need=1)]}], c["x_bank"], c["y_bank"], c["labels"], protect)
            assert np.array_equal(bits(xo), bits(x)) and np.array_equal(bits(yo), bits(y))
            # its own bleed is protected: nothing lands (the L's foot, 1.2 >= 1.05, too); without protect the whole lesion does
            assert landed[0, 0] == (0 if protect else lesion[2]) and counts.tolist() == ([0, 0] if protect else [1, int(lesion[2])])
    # a pure shift onto plain brain is a slice assignment
    kr = c["kr"]
    x, y = c["x"][:1], c["y"][:1]
    xo, yo, landed, counts, _ = R.paste(x, y, [{"active": 1, "n": 1, "items": [R.item(A, dr=kr, dc=0)]}], c["x_bank"], c["y_bank"], c["labels"], True)
    r0, c0, r1, c1 = (int(v) for v in A[3:])
    wx, wy = x.copy(), y.copy()
    wx[0, r0 + kr:r1 + kr + 1, c0:c1 + 1] = c["x_bank"][0, r0:r1 + 1, c0:c1 + 1]
    wy[0, r0 + kr:r1 + kr + 1, c0:c1 + 1] = c["y_bank"][0, r0:r1 + 1, c0:c1 + 1]
    assert np.array_equal(bits(xo), bits(wx)) and np.array_equal(bits(yo), bits(wy)) and landed[0, 0] == A[2] and counts.tolist() == [1, int(A[2])]
    assert np.isnan(xo[0, r0 + kr, c0, 0]) and bits(xo)[0, r0 + kr, c0, 0] == bits(c["x_bank"])[0, r0, c0, 0]       # the donor's NaN, payload included
    # and its mirror image is the flipped slice
    xo, yo, _, _, _ = R.paste(x, y, [{"active": 1, "n": 1, "items": [R.item(A, dr=kr, dc=c0 - (W - 1 - c1), flip=1)]}], c["x_bank"], c["y_bank"], c["labels"], True)
    wx, wy = x.copy(), y.copy()
    wx[0, r0 + kr:r1 + kr + 1, c0:c1 + 1] = c["x_bank"][0, r0:r1 + 1, c0:c1 + 1][:, ::-1]
    wy[0, r0 + kr:r1 + kr + 1, c0:c1 + 1] = c["y_bank"][0, r0:r1 + 1, c0:c1 + 1][:, ::-1]
    assert np.array_equal(bits(xo), bits(wx)) and np.array_equal(bits(yo), bits(wy))


# ------------------------------------------------------------------------------------------------ structs and symbols
SIZES = {"int32_t": 4, "UssegPasteItem": 40}


def _header():
    return open(os.path.join(ROOT, "include", "usseg_paste.h")).read()


def _header_layout(name):
    """(offsets by field, sizeof) of ``typedef struct <name> { ... }`` in the header text; every member is int32 or made of them."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, offsets = 0, {}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        for field in (n.strip() for n in names.split(",")):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", field)
            offsets[m.group(1)] = off
            off += SIZES[ctype] * (4 if m.group(2) == "USSEG_PASTE_MAX_ITEMS" else int(m.group(2) or 1))
    return offsets, off


def test_the_header_parses_and_the_structs_match_its_text():
    from ultrasound_modeling_amd import _abi, _lib as L
    abi = _abi.parse(_header(), "usseg_paste.h")
    assert tuple(abi.protos) == ("usseg_lesion_paste",) == L.PASTE_SYMBOLS
    assert list(abi.structs) == ["UssegPasteItem", "UssegPasteSample", "UssegPasteDesc"] and list(abi.consts.items()) == [("USSEG_PASTE_MAX_ITEMS", 4)]
    assert "#define USSEG_PASTE_MAX_ITEMS 4" in _header() and L.PASTE_MAX_ITEMS == 4
    res, args = abi.protos["usseg_lesion_paste"]
    assert res is C.c_int and len(args) == 12 and args[1] is C.c_void_p and args[0] is not C.c_void_p      # the device table is never dereferenced
    for name, cls in (("UssegPasteItem", L.PasteItem), ("UssegPasteSample", L.PasteSample), ("UssegPasteDesc", L.PasteDesc)):
        offsets, size = _header_layout(name)
        assert C.sizeof(cls) == size, name
        assert [f[0] for f in cls._fields_] == list(offsets), name
        for f in cls._fields_:
            assert getattr(cls, f[0]).offset == offsets[f[0]], (name, f[0])
    assert C.sizeof(L.PasteItem) == 40 and C.sizeof(L.PasteSample) == 168 and C.sizeof(L.PasteDesc) == 28
    assert [f[0] for f in L.PasteItem._fields_][:6] == ["record", "comp", "dr", "dc", "flip", "need"]
    assert "usseg_lesion_paste" not in L.EXPORTED_SYMBOLS                      # the fifth Abi is its own


def test_the_symbol_is_exported_and_the_source_is_built():
    from ultrasound_modeling_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "usseg_lesion_paste")
    fn = lib.usseg_lesion_paste
    assert (fn.restype, list(fn.argtypes)) == _lib.PASTE_ABI.protos["usseg_lesion_paste"]
    mk = open(os.path.join(ROOT, "ultrasound_modeling_amd", "csrc", "Makefile")).read()
    for var in ("SRCS", "NOPK_SRCS"):
        assert sum("paste.hip" in line.split() for line in mk.splitlines() if line.startswith(var + " ")) == 1, var
    assert any(line.startswith("%.o:") and "usseg_paste.h" in line for line in mk.splitlines())
    from ultrasound_modeling_amd import paste as Pp

    t = Pp.sample_table(R.case((12, 9, 2), np.float32)["tables"][0], "cpu")    # the table's bytes, without a device
    assert t.numel() == 6 * 168
    arr = (_lib.PasteSample * 6).from_buffer_copy(bytes(t.numpy()))
    it = R.case((12, 9, 2), np.float32)["tables"][0][0]["items"][1]
    got = arr[0].items[1]
    assert (arr[0].active, arr[0].n_items, arr[5].active, arr[4].n_items) == (1, 2, 0, 0)
    assert (got.record, got.comp, got.dr, got.dc, got.flip, got.need, got.r0, got.c0, got.r1, got.c1) == (
        it["record"], it["comp"], it["dr"], it["dc"], it["flip"], it["need"], *it["box"])


# ------------------------------------------------------------------------------------------------ argument checks (no launch: no device needed)
PTRS = dict(samples=0x1000, x=0x100000, y=0x200000, x_bank=0x300000, y_bank=0x400000, labels=0x500000, x_out=0x600000, y_out=0x700000,
            landed=0x800000, counts=0x900000)


def _paste(B=1, H=4, W=4, C_=3, f64=1, N=2, protect=1, null_desc=False, **ptrs):
    from ultrasound_modeling_amd import _lib as L
    lib = L.load()
    p = dict(PTRS, **ptrs)
    d = None if null_desc else C.byref(L.PasteDesc(B, H, W, C_, f64, N, protect))
    rc = lib.usseg_lesion_paste(d, p["samples"], p["x"], p["y"], p["x_bank"], p["y_bank"], p["labels"], p["x_out"], p["y_out"], p["landed"], p["counts"], None)
    return rc, lib.usseg_last_error()


def test_lesion_paste_rejects_bad_arguments():
    assert _paste(null_desc=True)[0] == -1
    for name in PTRS:
        rc, msg = _paste(**{name: None})
        assert rc == -1 and b"lesion_paste: null pointer" in msg, name
    for kw in (dict(B=0), dict(H=0), dict(W=-3), dict(C_=0), dict(N=0), dict(N=-1)):
        rc, msg = _paste(**kw)
        assert rc == -1 and b"lesion_paste: bad descriptor (B, H, W, C, N >= 1)" in msg, kw
    for kw in (dict(B=1 << 15, H=1 << 15, W=2, C_=1), dict(B=1 << 10, H=1 << 10, W=1 << 10, C_=2), dict(B=1 << 30, H=4, W=1, C_=1),
               dict(B=1 << 30, H=1 << 30, W=1 << 30, C_=1 << 30), dict(B=1, H=1 << 15, W=1 << 15, C_=2)):
        rc, msg = _paste(**kw)
        assert rc == -1 and b"B*H*W*C < 2^31" in msg, kw
    rc, msg = _paste(B=1 << 29, H=1, W=1, C_=1)
    assert rc == -1 and b"B < 2^29" in msg
    rc, msg = _paste(B=1, H=1 << 15, W=1 << 14, C_=3, N=(1 << 31) - 1)
    assert rc == -1 and b"N*H*W*C*8 <= 2^62" in msg
    for name in ("x", "x_bank", "x_out"):
        rc, msg = _paste(**{name: PTRS[name] + 4})
        assert rc == -1 and b"aligned to their element (8 bytes)" in msg, name
        rc, msg = _paste(f64=0, **{name: PTRS[name] + 2})
        assert rc == -1 and b"aligned to their element (4 bytes)" in msg, name
    for name in ("y", "y_bank", "labels", "y_out", "landed", "samples"):
        rc, msg = _paste(**{name: PTRS[name] + 2})
        assert rc == -1 and b"4-byte aligned" in msg, name
    rc, msg = _paste(counts=PTRS["counts"] + 4)
    assert rc == -1 and b"counts must be 8-byte aligned" in msg
    xb, yb, bank_x, bank_y = 4 * 4 * 3 * 8, 4 * 4 * 4, 2 * 4 * 4 * 3 * 8, 2 * 4 * 4 * 4
    for kw in (dict(x_out=PTRS["x"]), dict(y_out=PTRS["y"]), dict(x_out=PTRS["x"] + xb - 8), dict(x_out=PTRS["x"] - xb + 8), dict(x_out=PTRS["y"]),
               dict(y_out=PTRS["x"] + 8), dict(y_out=PTRS["y"] + yb - 4),
               dict(x_out=PTRS["x_bank"] + bank_x - 8), dict(y_out=PTRS["y_bank"] + bank_y - 4), dict(x_out=PTRS["labels"] + bank_y - 8),
               dict(y_out=PTRS["labels"]), dict(landed=PTRS["x_bank"] + xb), dict(landed=PTRS["y"] + 8), dict(counts=PTRS["labels"] + 8),
               dict(counts=PTRS["samples"] + 160), dict(landed=PTRS["samples"] - 12), dict(y_out=PTRS["samples"] + 164), dict(counts=PTRS["x"] + xb - 8)):
        rc, msg = _paste(**kw)
        assert rc == -1 and b"must not overlap x / y, the bank or the sample table" in msg, kw
    for kw in (dict(y_out=PTRS["x_out"] + xb - 4), dict(landed=PTRS["x_out"]), dict(counts=PTRS["y_out"] + yb - 8), dict(counts=PTRS["landed"] + 8),
               dict(landed=PTRS["counts"] + 12)):
        rc, msg = _paste(**kw)
        assert rc == -1 and b"must not overlap each other" in msg, kw
    rc, msg = _paste(x_out=PTRS["x"] + xb // 2 - 4, f64=0)                     # fp32 x is half as long: its last element
    assert rc == -1 and b"must not overlap" in msg


def test_python_surface_refuses_host_tensors_and_bad_shapes():
    import torch
    from ultrasound_modeling_amd import paste as Pp
    x, y = torch.zeros(1, 4, 4, 3, dtype=torch.float64), torch.zeros(1, 4, 4)
    xb, yb, lb = torch.zeros(2, 4, 4, 3, dtype=torch.float64), torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Pp.lesion_paste(x, y, torch.zeros(168, dtype=torch.uint8), xb, yb, lb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Pp.LesionBank(yb)
    bank = Pp.LesionBank(labels=lb, table=[[0, 1, 4, 0, 0, 1, 1]])
    with pytest.raises(ValueError, match="parameter sets"):
        Pp.paste_batch(x, y, [], Pp.paste_config(), bank, xb, yb)
