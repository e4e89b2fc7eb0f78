"""ctypes binding of libusseg_hip.so, generated at import from the C ABI declared in include/usseg.h and, for the evaluator's score kernels,
include/usseg_scores.h, for the distillation loss, include/usseg_distill.h, for gradient accumulation, include/usseg_accumulate.h and, for the
lesion copy-paste augmentation, include/usseg_paste.h (_abi.py reads all five; ``ABI`` is the first header's, ``SCORES_ABI`` the second's,
``DISTILL_ABI`` the third's, ``GRAD_ACC_ABI`` the fourth's, ``PASTE_ABI`` the fifth's).

There is NO fallback: if the header or the shared library is missing or a call fails, an exception is raised.
Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: the HIP runtime torch loads is the one this library must share)
from . import _abi, knobs

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = knobs.get("USSEG_LIB") or os.path.join(_HERE, "libusseg_hip.so")   # USSEG_LIB: a diagnostic build of the SAME sources (tools/diag_norm_variants.sh)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "usseg.h")
SCORES_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "usseg_scores.h")
DISTILL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "usseg_distill.h")
GRAD_ACC_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "usseg_accumulate.h")
PASTE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "usseg_paste.h")

c_i32, c_i64, c_f32, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class UssegError(RuntimeError):
    pass


def read_header(path: str = HEADER_PATH) -> _abi.Abi:
    if not os.path.exists(path):
        raise UssegError(f"{path} not found: the binding is read from the header, which lies in include/ beside the package directory")
    with open(path) as f:
        return _abi.parse(f.read(), path)


ABI = read_header()

# every struct under the header's name without "Usseg" (ConvDesc, LossDesc, WgradDst, PackJob, ...) and every #define and enumerator
# under its name without "USSEG_" (ACT_LRELU, OUT_F32, ACCUMULATE, SEG_COUNTS, SCHED_MAX_PIECES, ...)
globals().update({cls.__name__: cls for cls in ABI.structs.values()})
globals().update({name[len("USSEG_"):]: value for name, value in ABI.consts.items()})
TEMP_NLL_UNIT = 2.0 ** -20    # one count of usseg_temperature_nll's sums (the header states it in prose only)

_PROTOS = ABI.protos    # name: (restype, argtypes)
EXPORTED_SYMBOLS = tuple(_PROTOS)

# the second header (csrc/scores.hip): its own Abi, so that ABI, _PROTOS and EXPORTED_SYMBOLS stay the first header's alone
SCORES_ABI = read_header(SCORES_HEADER_PATH)
SCORES_SYMBOLS = tuple(SCORES_ABI.protos)
SCORES_MEASURE_FIELDS, SCORES_EMPTY_MIN = SCORES_ABI.consts["USSEG_SCORES_MEASURE_FIELDS"], SCORES_ABI.consts["USSEG_SCORES_EMPTY_MIN"]
SCORES_BOOT_MAX_K, SCORES_BOOT_MAX = SCORES_ABI.consts["USSEG_SCORES_BOOT_MAX_K"], SCORES_ABI.consts["USSEG_SCORES_BOOT_MAX"]

# the third header (csrc/distill.hip): likewise its own Abi, with its own struct and constants
DISTILL_ABI = read_header(DISTILL_HEADER_PATH)
DISTILL_SYMBOLS = tuple(DISTILL_ABI.protos)
DistillDesc = DISTILL_ABI.structs["UssegDistillDesc"]
DISTILL_ACC_FLOATS, DISTILL_SETTINGS = DISTILL_ABI.consts["USSEG_DISTILL_ACC_FLOATS"], DISTILL_ABI.consts["USSEG_DISTILL_SETTINGS"]

# the fourth header (csrc/accumulate.hip): one entry point, no struct, no constant
GRAD_ACC_ABI = read_header(GRAD_ACC_HEADER_PATH)
GRAD_ACC_SYMBOLS = tuple(GRAD_ACC_ABI.protos)

# the fifth header (csrc/paste.hip): one entry point, the sample table's structs and the item limit
PASTE_ABI = read_header(PASTE_HEADER_PATH)
PASTE_SYMBOLS = tuple(PASTE_ABI.protos)
PasteItem, PasteSample, PasteDesc = (PASTE_ABI.structs[n] for n in ("UssegPasteItem", "UssegPasteSample", "UssegPasteDesc"))
PASTE_MAX_ITEMS = PASTE_ABI.consts["USSEG_PASTE_MAX_ITEMS"]

_lib = None


def bind(lib: C.CDLL, names=EXPORTED_SYMBOLS, protos=None) -> C.CDLL:
    """Give the named entry points of ``lib`` (any build of these sources) the prototypes of ``protos`` (default: usseg.h's)."""
    protos = _PROTOS if protos is None else protos
    for name in names:
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype, fn.argtypes = protos[name]
    return lib


def load() -> C.CDLL:
    """Load libusseg_hip.so (built by ``__graft_entry__.build()`` / ``make -C ultrasound_modeling_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UssegError(f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                         f"g.build()'). There is no CPU fallback.")
    _lib = bind(bind(bind(C.CDLL(LIB_PATH)), SCORES_SYMBOLS, SCORES_ABI.protos), DISTILL_SYMBOLS, DISTILL_ABI.protos)
    bind(_lib, GRAD_ACC_SYMBOLS, GRAD_ACC_ABI.protos)
    bind(_lib, PASTE_SYMBOLS, PASTE_ABI.protos)
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().usseg_last_error().decode("utf-8", "replace")
        raise UssegError(f"{what}: usseg error {rc}: {msg}")
