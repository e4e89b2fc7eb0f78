"""CPU tests of the binding that ultrasound_modeling_amd/_abi.py reads out of include/usseg.h: the reader's known answers on a small header
written here, what it must refuse, and pins on the real header - prototypes, struct layouts, job-table record types and the optimiser's
checkpoint words - typed in as literals from the hand-written binding this one replaced.  Nothing here needs a GPU or the built library."""
import ctypes as C
import os

import numpy as np
import pytest

from ultrasound_modeling_amd import _abi, _lib as L, flat
from ultrasound_modeling_amd.schedules import PiecewiseConstantDecay

i32, i64, u32, u64, f32, f64, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_void_p

SMALL = """
/* a comment with a ; and a { in it */
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* stream_t; // a line comment
#define N_MAX 4
#define ROWS 0x2 /* hex */
typedef enum UssegKind { KIND_A = 0, KIND_B = -3 } UssegKind;
enum {
  FLAG_ONE = 1,
  FLAG_TWO = 2
};
typedef struct UssegInner {
  int32_t B, H, W;      /* several declarators */
  float alpha;
} UssegInner;
typedef struct UssegOuter {
  UssegInner in;               /* nested by value */
  const float *g, *b;          /* pointer fields */
  const UssegInner* link;      /* typed pointer */
  int32_t grid[N_MAX][ROWS];   /* two-dimensional */
  UssegInner many[N_MAX - 1];  /* array of structs */
  uint64_t seed;
  double rot[6];
  uint8_t tag;
} UssegOuter;
const char* small_error(void);
int64_t small_bytes(int64_t n, int32_t c);
int small_run(const UssegOuter* d, UssegInner by_value, const UssegOuter* jobs_dev, const float* x, void* const* members,
              uint32_t mask, uint64_t seed, double r, float a, stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_known_answers():
    abi = _abi.parse(SMALL, "small.h")
    assert abi.consts == {"N_MAX": 4, "ROWS": 2, "KIND_A": 0, "KIND_B": -3, "FLAG_ONE": 1, "FLAG_TWO": 2}
    assert list(abi.structs) == ["UssegInner", "UssegOuter"]
    inner, outer = abi.structs["UssegInner"], abi.structs["UssegOuter"]
    assert (inner.__name__, outer.__name__) == ("Inner", "Outer")
    assert inner._fields_ == [("B", i32), ("H", i32), ("W", i32), ("alpha", f32)] and C.sizeof(inner) == 16
    assert outer._fields_ == [("in", inner), ("g", vp), ("b", vp), ("link", C.POINTER(inner)), ("grid", (i32 * 2) * 4), ("many", inner * 3),
                              ("seed", u64), ("rot", f64 * 6), ("tag", C.c_uint8)]
    assert [getattr(outer, n).offset for n, _ in outer._fields_] == [0, 16, 24, 32, 40, 72, 120, 128, 176]
    assert C.sizeof(outer) == 184                                    # one uint8_t, padded to the 8-byte alignment
    assert abi.protos == {"small_error": (C.c_char_p, []), "small_bytes": (i64, [i64, i32]),
                          "small_run": (C.c_int, [C.POINTER(outer), inner, vp, vp, vp, u32, u64, f64, f32, vp])}
    o = outer(inner(1, 2, 3, 0.5), None, None, None, ((1, 2), (3, 4)))          # positional and nested construction, as ops.py does
    assert (o.grid[1][0], getattr(o, "in").W) == (3, 3)


@pytest.mark.parametrize("decl,offending", [
    ("typedef struct UssegA { unsigned x; } UssegA;", "unsigned"),                      # unknown type
    ("int f(struct Foo* p);", "struct"),                                                # unknown type in a parameter
    ("typedef struct UssegA { void (*cb)(int); } UssegA;", "void (*cb)(int)"),          # function pointer field
    ("int f(int (*cb)(int), int32_t n);", "int f(int (*cb)(int), int32_t n)"),          # function pointer parameter
    ("typedef struct UssegA { int32_t a : 3; } UssegA;", "int32_t a : 3"),              # bit-field
    ("typedef struct UssegA { int32_t a[UNKNOWN_N]; } UssegA;", "UNKNOWN_N"),           # array size: not a known constant
    ("typedef struct UssegA { int32_t a[sizeof(int)]; } UssegA;", "a[sizeof(int)]"),    # array size: not a literal
    ("typedef struct UssegA { int32_t a; } UssegA;\nint f(int32_t a, ", "int f(int32_t a,"),   # truncated declaration
    ("typedef struct UssegA { int32_t a;", "typedef struct UssegA"),                    # truncated struct
    ("typedef struct UssegA { int32_t a } UssegA;", "int32_t a"),                       # a field without its semicolon
    ("int f(int32_t);", "int f(int32_t)"),                                              # a parameter without a name
    ("#define HALF 0.5", "#define HALF 0.5"),                                           # a define that is no integer
    ("enum { A, B };", "A"),                                                            # enumerators without values
    ("int32_t* f(void);", "int32_t* f(void)"),                                          # a pointer return that is not char*
])
def test_reader_refuses(decl, offending):
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse("#define KNOWN 2\n" + decl, "bad.h")
    assert offending in str(e.value) and "bad.h:" in str(e.value), str(e.value)


def test_reader_names_the_line():
    with pytest.raises(_abi.AbiError, match=r"bad\.h:4: unknown type 'long'"):
        _abi.parse("/* one\n two */\nint f(void);\nint g(long n);\n", "bad.h")


def test_missing_header_is_an_error_with_the_path(tmp_path):
    with pytest.raises(L.UssegError, match="nowhere/usseg.h"):
        L.read_header(str(tmp_path / "nowhere" / "usseg.h"))
    assert L.HEADER_PATH == os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))), "include", "usseg.h")


# ------------------------------------------------------------------------------------------------ pins on the real header
_NAMES = {i32: "i32", i64: "i64", u32: "u32", u64: "u64", f32: "f32", f64: "f64", vp: "vp", C.c_char_p: "char_p", C.c_uint8: "u8"}


def _name(t):
    if t in _NAMES:
        return _NAMES[t]
    if hasattr(t, "_length_"):
        return f"{_name(t._type_)}[{t._length_}]"
    if hasattr(t, "contents"):
        return f"P({_name(t._type_)})"
    return t.__name__


def test_header_counts_and_names():
    assert (len(L.ABI.protos), len(L.ABI.structs)) == (167, 34)
    assert all(n.startswith("Usseg") and getattr(L, n[5:]) is c for n, c in L.ABI.structs.items())
    assert L.EXPORTED_SYMBOLS == tuple(L._PROTOS) and all(n.startswith("usseg_") for n in L.EXPORTED_SYMBOLS)
    assert (L.ACT_NONE, L.ACT_LRELU, L.ACT_RELU, L.ACT_ELU, L.ACT_GELU, L.OUT_F32, L.ACCUMULATE) == (0, 1, 2, 3, 4, 1, 2)
    assert (L.OK, L.ERR_BAD_ARG, L.ERR_UNSUPPORTED, L.ERR_LAUNCH) == (0, -1, -2, -3)
    assert (L.ACC_FLOATS, L.SEG_COUNTS, L.OVERLAP_ACC_FLOATS, L.SORT_TILE, L.SORT_DIGIT_BITS, L.SCHED_MAX_PIECES) == (2050, 23, 8224, 2048, 8, 16)
    assert (L.AVERAGE_OFF, L.AVERAGE_EMA, L.AVERAGE_SWA, L.PREP_H, L.PREP_W, L.PREP_AUG_PARTIALS) == (0, 1, 2, 256, 80, 64)
    assert (L.ENSEMBLE_MAX, L.CALIB_MAX_BINS, L.SWEEP_MAX_BINS, L.TEMP_MAX_BETAS, L.TEMP_NLL_CAP, L.WARP_MAX_RADIUS) == (16, 64, 4096, 16, 1024, 64)


# (restype, argtypes).  Two differ from the hand-written table on purpose: usseg_conv2d_wgrad_multi took "i32 vp vp i64 vp" (its caller passed
# an address, now the array itself) and usseg_ensemble_merge took P(vp) for its host array of pointers (vp accepts the same ctypes array).
PROTOS = {
    "usseg_last_error": ("char_p", ""),
    "usseg_topk_select_ws_bytes": ("i64", "i64"),
    "usseg_dropout_mask": ("i32", "vp i64 i32 i32 u64 f32 vp"),
    "usseg_cone_index": ("i32", "vp vp i32 i32 f64 f64 f64 i32 i32 vp vp"),
    "usseg_lovasz_coeffs": ("i32", "P(LossDesc) LovaszLoss vp vp vp vp vp i64 vp"),
    "usseg_ensemble_merge": ("i32", "P(EnsembleDesc) vp u32 vp vp vp vp vp"),
    "usseg_adamw_avg_step": ("i32", "vp vp vp vp vp i64 vp f32 vp vp vp f32 f32 f32 vp vp vp"),
    "usseg_conv2d_wgrad_multi": ("i32", "i32 P(WgradJob) vp i64 vp"),
    "usseg_pack_weights_batched": ("i32", "vp i32 vp"),           # jobs_dev: a device table stays untyped
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_prototype_pins(name):
    res, args = L._PROTOS[name]
    assert (_name(res), " ".join(_name(a) for a in args)) == PROTOS[name]


LAYOUTS = {
    "ConvDesc": (48, "B:i32@0 H:i32@4 W:i32@8 Cin:i32@12 Cout:i32@16 ldx:i32@20 ldy:i32@24 ksize:i32@28 dilation:i32@32 act:i32@36 alpha:f32@40 "
                     "flags:i32@44"),
    "ConvJob": (104, "desc:ConvDesc@0 x:vp@48 wp:vp@56 bias:vp@64 residual:vp@72 ldr:i32@80 reserved:i32@84 y:vp@88 scale:vp@96"),
    "WgradDst": (200, "nblocks:i32@0 reserved:i32@4 blk:WgradBlock[4]@8"),
    "WgradBlock": (48, "dst:vp@0 sT:i64@8 sI:i64@16 sO:i64@24 i_off:i32@32 o_off:i32@36 ni:i32@40 no:i32@44"),
    "WgradJob": (80, "desc:ConvDesc@0 x:vp@48 dy:vp@56 dw:vp@64 dst:P(WgradDst)@72"),
    "PrepAugSample": (120, "do_flip:i32@0 do_reduc:i32@4 do_contrast:i32@8 do_clip:i32@12 clip:i32[4]@16 do_rotate:i32@32 rot_slot:i32@36 "
                           "do_shift:i32@40 shift_r:i32@44 shift_c:i32@48 shift_dir:i32@52 do_noise:i32@56 reserved:i32@60 seed:u64@64 rot:f64[6]@72"),
    "AugSample": (72, "do_reduc:i32@0 nclip:i32@4 clip:i32[4][2]@8 do_shift:i32@40 shift_r:i32@44 shift_c:i32@48 shift_dir:i32@52 do_noise:i32@56 "
                      "do_flip:i32@60 seed:u64@64"),
    "LrSchedule": (192, "n:i32@0 boundary:i32[15]@4 lr:f32[16]@64 wd:f32[16]@128"),
    "Average": (20, "mode:i32@0 decay:f32@4 dynamic_decay:i32@8 start:i32@12 period:i32@16"),
    "PackJob": (80, "src:vp@0 dst:vp@8 sT:i64@16 sN:i64@24 sK:i64@32 T:i32@40 Nn:i32@44 Kk:i32@48 Kw:i32@52 tap_stride:i32@56 n_off:i32@60 "
                    "k_off:i32@64 reserved:i32@68 nscale:vp@72"),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layout_pins(name):
    cls = getattr(L, name)
    assert (C.sizeof(cls), " ".join(f"{n}:{_name(t)}@{getattr(cls, n).offset}" for n, t in cls._fields_)) == LAYOUTS[name]


# the record types ops.py wrote out by hand: (name, format, offset) of every field, and the item size
JOB_TABLES = {
    "PackJob": (80, [("src", "<u8", 0), ("dst", "<u8", 8), ("sT", "<i8", 16), ("sN", "<i8", 24), ("sK", "<i8", 32), ("T", "<i4", 40), ("Nn", "<i4", 44),
                     ("Kk", "<i4", 48), ("Kw", "<i4", 52), ("tap_stride", "<i4", 56), ("n_off", "<i4", 60), ("k_off", "<i4", 64), ("reserved", "<i4", 68),
                     ("nscale", "<u8", 72)]),
    "UnpackJob": (80, [("scratch", "<u8", 0), ("dst", "<u8", 8), ("sT", "<i8", 16), ("sN", "<i8", 24), ("sK", "<i8", 32), ("Mrows", "<i4", 40),
                       ("Ncols", "<i4", 44), ("T", "<i4", 48), ("Nn", "<i4", 52), ("Kk", "<i4", 56), ("n_off", "<i4", 60), ("k_off", "<i4", 64),
                       ("accumulate", "<i4", 68), ("scale", "<f4", 72), ("reserved", "<i4", 76)]),
    "BnFoldJob": (72, [("gamma", "<u8", 0), ("beta", "<u8", 8), ("mean", "<u8", 16), ("var", "<u8", 24), ("bias", "<u8", 32), ("scale", "<u8", 40),
                       ("shift", "<u8", 48), ("C", "<i4", 56), ("Cp", "<i4", 60), ("eps", "<f4", 64), ("reserved", "<i4", 68)]),
}


@pytest.mark.parametrize("name", sorted(JOB_TABLES))
def test_job_table_record_types(name):
    from ultrasound_modeling_amd import ops
    dt = {"PackJob": ops.PACK_JOB_DTYPE, "UnpackJob": ops.UNPACK_JOB_DTYPE, "BnFoldJob": ops.BN_FOLD_JOB_DTYPE}[name]
    size, fields = JOB_TABLES[name]
    assert dt == np.dtype(getattr(L, name)) and dt.itemsize == size
    assert [(n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names] == fields


def test_job_table_bytes():
    """One pack job through the record type gives the bytes of the C struct, field by field."""
    from ultrasound_modeling_amd import ops
    job = (0x1122334455667788, 0x10, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 0, 0x20)
    raw = np.array([job], dtype=ops.PACK_JOB_DTYPE).tobytes()
    assert raw == bytes(L.PackJob(*job)) and len(raw) == 80
    assert raw[:8] == bytes.fromhex("8877665544332211") and raw[40:44] == (9).to_bytes(4, "little") and raw[72:] == (0x20).to_bytes(8, "little")


def test_checkpoint_words_of_the_schedule_table():
    """The int32 image of UssegLrSchedule that a checkpoint holds, word for word as the hand-indexed table wrote it."""
    t = flat._table(PiecewiseConstantDecay([100, 250, 1000], [1e-3, 5e-4, 2.5e-4, 1e-5]), PiecewiseConstantDecay([250, 4000], [0.01, 0.004, 0.0]))
    want = np.zeros(48, dtype=np.int32)
    want[:5] = [5, 100, 250, 1000, 4000]
    want[16:21] = [981668463, 973279855, 964891247, 925353388, 925353388]
    want[32:36] = [1008981770, 1008981770, 998445679, 998445679]
    assert t.dtype == np.int32 and t.shape == (48,) and np.array_equal(t, want)
    lr, wd = flat._from_table(want)
    assert lr.boundaries == wd.boundaries == (100, 250, 1000, 4000)
    assert lr.values.tolist() == [np.float32(v) for v in (1e-3, 5e-4, 2.5e-4, 1e-5, 1e-5)]
    assert wd.values.tolist() == [np.float32(v) for v in (0.01, 0.01, 0.004, 0.004, 0.0)]
    one = flat._table(3e-4, None)
    assert one.nonzero()[0].tolist() == [0, 16] and (int(one[0]), int(one[16])) == (1, 966609234)
    assert flat._from_table(one) == (float(np.float32(3e-4)), 0.0)


def test_checkpoint_words_of_the_average_descriptor():
    ema = flat._average_words(flat.average_config({"mode": "ema", "decay": 0.999, "dynamic_decay": True, "start_step": 7}))
    swa = flat._average_words(flat.average_config({"mode": "swa", "start": 40, "period": 5}))
    assert ema.dtype == swa.dtype == np.int32
    assert ema.tolist() == [1, 1065336439, 1, 7, 1] and swa.tolist() == [2, 0, 0, 40, 5]
    assert flat._average_from_words(ema) == {"mode": "ema", "decay": float(np.float32(0.999)), "dynamic_decay": True, "start_step": 7}
    assert flat._average_from_words(swa) == {"mode": "swa", "start": 40, "period": 5}
