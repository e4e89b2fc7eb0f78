// Every USSEG_* environment switch the kernel library reads: one line each, read through knob<K_...>() and nowhere else
// (tests/test_cpu_knobs.py reads this table as text; DESIGN.md section 4d documents it with the switches of the Python side).
//   kind      INT: unset -> default, else atoll() of the value ("junk" parses to 0).  PRESENT: 1 if the variable exists, whatever it holds.
//   lifetime  ONCE: read at the first use of THAT switch and kept for the process (tools and tests set these after the library is
//             loaded and before the first launch).  PER_CALL: read at every use - the tests flip exactly these inside one process.
// Why a default has its value is written where the planner uses it.
#pragma once
#include <stdint.h>
#include <stdlib.h>

// clang-format off
#define USSEG_KNOBS(X)                                                                                                                  \
  /* conv_big.hip */                                                                                                                    \
  X(K_BIG,                "USSEG_BIG",                INT,     1,     ONCE,     "0: conv_big and the streaming conv take no launch")        \
  X(K_BIG_PX,             "USSEG_BIG_PX",             INT,     0,     ONCE,     "conv_big: force the pixel tile (128 / 256; 0: planner)")   \
  X(K_BIG_NT,             "USSEG_BIG_NT",             INT,     0,     ONCE,     "conv_big: force the channel tile (1 / 2 / 4 x 16; 0: planner)") \
  X(K_BIG_MIN_WG,         "USSEG_BIG_MIN_WG",         INT,     128,   ONCE,     "conv_big: smallest launch it takes, in workgroups")        \
  X(K_BIG_WG_TILE,        "USSEG_BIG_WG_TILE",        INT,     512,   ONCE,     "conv_big: narrow the channel tile below this many workgroups") \
  X(K_BIG_MIN_CIN,        "USSEG_BIG_MIN_CIN",        INT,     33,    ONCE,     "conv_big: fewest input channels of a pass it takes")       \
  X(K_BIG_STAGES,         "USSEG_BIG_STAGES",         INT,     0,     ONCE,     "conv_big LDS stages: 0 by launch size, 1 / 2 forced")      \
  X(K_BIG_W8,             "USSEG_BIG_W8",             INT,     1,     PER_CALL, "256-pixel tile on eight waves: 0 never, 1 planner, 2 forced") \
  X(K_BIG_W8_MIN,         "USSEG_BIG_W8_MIN",         INT,     128,   ONCE,     "fewest workgroups left for the eight-wave tile")           \
  X(K_STREAM,             "USSEG_STREAM",             INT,     1,     ONCE,     "0: the streaming conv takes no launch")                    \
  X(K_STREAM_PX,          "USSEG_STREAM_PX",          INT,     0,     ONCE,     "streaming conv: force the pixel tile (128 / 256; 0: planner)") \
  X(K_STREAM_MIN_STEPS,   "USSEG_STREAM_MIN_STEPS",   INT,     1,     PER_CALL, "streaming conv: fewest K steps per workgroup it takes")    \
  X(K_STREAM_WGX,         "USSEG_STREAM_WGX",         INT,     0,     PER_CALL, "streaming conv: force grid.x (>= 8, rounded down to a multiple of 8)") \
  X(K_STREAM_OCC,         "USSEG_STREAM_OCC",         INT,     0,     ONCE,     "streaming conv: cap on workgroups per CU (0: by LDS)")     \
  X(K_STREAM_RES,         "USSEG_STREAM_RES",         INT,     1,     ONCE,     "0: passes with a residual do not stream")                  \
  X(K_STREAM_MULTI,       "USSEG_STREAM_MULTI",       INT,     1,     ONCE,     "0: multi-job launches do not stream")                      \
  X(K_STREAM_MERGE,       "USSEG_STREAM_MERGE",       INT,     1,     PER_CALL, "streaming jobs of one plan in one launch (0: a launch per job)") \
  /* conv_halo.hip, wgrad_halo.hip */                                                                                                   \
  X(K_NO_HALO,            "USSEG_NO_HALO",            PRESENT, 0,     ONCE,     "the halo-tile conv and weight-gradient kernels take no launch") \
  X(K_NO_PERSIST,         "USSEG_NO_PERSIST",         PRESENT, 0,     ONCE,     "conv_halo: never the persistent variant")                  \
  X(K_PERSIST_OCC,        "USSEG_PERSIST_OCC",        INT,     0,     ONCE,     "persistent conv_halo: workgroups per CU (0: by LDS)")      \
  /* conv_igemm.hip */                                                                                                                  \
  X(K_IGEMM_WG_MIN,       "USSEG_IGEMM_WG_MIN",       INT,     256,   ONCE,     "igemm: narrow the channel tile below this many workgroups") \
  X(K_IGEMM_KC,           "USSEG_IGEMM_KC",           INT,     0,     ONCE,     "register-staged igemm: force the K step (4 / 8 chunks; 0: by K length)") \
  X(K_IGEMM_DMA,          "USSEG_IGEMM_DMA",          INT,     1,     ONCE,     "0: never the LDS-DMA igemm")                               \
  X(K_IGEMM_DMA_MIN,      "USSEG_IGEMM_DMA_MIN",      INT,     4,     ONCE,     "LDS-DMA igemm: fewest K chunks it takes")                  \
  X(K_IGEMM_DMA_BATCHED,  "USSEG_IGEMM_DMA_BATCHED",  INT,     1,     ONCE,     "0: batched GEMMs stay on the register-staged igemm")       \
  X(K_IGEMM_XCD,          "USSEG_IGEMM_XCD",          INT,     1,     ONCE,     "XCD-aware item order: 0 off, 1 activation-heavy launches, 2 all") \
  X(K_IGEMM_PERSIST,      "USSEG_IGEMM_PERSIST",      INT,     1,     ONCE,     "0: never the persistent LDS-DMA igemm")                    \
  X(K_IGEMM_STAGES8,      "USSEG_IGEMM_STAGES8",      INT,     4,     ONCE,     "ring depth of sparse long-K 128-channel launches (2: off, 3, 4)") \
  X(K_IGEMM_STAGES8_WG,   "USSEG_IGEMM_STAGES8_WG",   INT,     256,   ONCE,     "largest launch, in workgroups, that gets the deeper ring") \
  /* wgrad.hip, wgrad_halo.hip */                                                                                                       \
  X(K_WGRAD_DMA,          "USSEG_WGRAD_DMA",          INT,     1,     ONCE,     "0: never the LDS-DMA per-tap weight gradient / batched TN GEMM") \
  X(K_WGRAD_TM,           "USSEG_WGRAD_TM",           INT,     0,     ONCE,     "per-tap wgrad: force the tile (1: 64x64, 2: 128x128; 0: planner)") \
  X(K_WGD_TARGET,         "USSEG_WGD_TARGET",         INT,     512,   ONCE,     "per-tap wgrad: workgroups the split-K aims for")           \
  X(K_WGD_CAP,            "USSEG_WGD_CAP",            INT,     4,     ONCE,     "per-tap wgrad: slab traffic cap, in multiples of the operand bytes") \
  X(K_WG_QUANT,           "USSEG_WG_QUANT",           INT,     1,     ONCE,     "0: no wave-quantisation search of the split count (both wgrad kernels)") \
  X(K_WGRAD_DEBUG,        "USSEG_WGRAD_DEBUG",        PRESENT, 0,     ONCE,     "print every weight-gradient plan to stderr")               \
  X(K_WGRAD_POW2,         "USSEG_WGRAD_POW2",         INT,     1,     ONCE,     "0: no shift decode of power-of-two grids")                 \
  X(K_WGRAD_XCD,          "USSEG_WGRAD_XCD",          INT,     1,     ONCE,     "0: no XCD-aware item order in the per-tap wgrad")          \
  X(K_WG_TARGET,          "USSEG_WG_TARGET",          INT,     256,   ONCE,     "halo wgrad: workgroups the split-K aims for")              \
  X(K_SLAB_CAP,           "USSEG_SLAB_CAP",           INT,     2,     ONCE,     "halo wgrad: slab traffic cap, in multiples of the operand bytes") \
  X(K_WGHALO_XCD,         "USSEG_WGHALO_XCD",         INT,     1,     ONCE,     "0: no XCD-aware item order in the halo wgrad")             \
  X(K_WGRAD_PF,           "USSEG_WGRAD_PF",           INT,     1,     ONCE,     "0: halo wgrad without the register prefetch")              \
  X(K_WGRAD_8W,           "USSEG_WGRAD_8W",           INT,     1,     ONCE,     "0: the 64x64 halo wgrad tile on four waves, not eight")    \
  X(K_TCONV_HALO,         "USSEG_TCONV_HALO",         INT,     0,     PER_CALL, "1: transposed-conv wgrad as four parity-class halo jobs")  \
  /* cardinal.hip */                                                                                                                    \
  X(K_CARD_BWD_G,         "USSEG_CARD_BWD_G",         INT,     0,     ONCE,     "fused cardinal backward: force the workgroup pairs (0: one resident wave)") \
  X(K_LN_TILE,            "USSEG_LN_TILE",            INT,     1,     ONCE,     "0: never the tile LayerNorm backward")                     \
  X(K_LN_PAIR,            "USSEG_LN_PAIR",            INT,     1,     ONCE,     "0: never the paired LayerNorm backward launch")            \
  X(K_LN_TILE_MIN,        "USSEG_LN_TILE_MIN",        INT,     32768, ONCE,     "fewest pixels for the tile / paired LayerNorm backward")   \
  /* flash_attn.hip, swin.hip, attn_loss_optim.hip */                                                                                   \
  X(K_FLASH_TILE,         "USSEG_FLASH_TILE",         INT,     -1,    ONCE,     "fused attention tiling 0 / 1 / 2 (-1: by problem size)")   \
  X(K_WINATTN_MFMA,       "USSEG_WINATTN_MFMA",       INT,     1,     ONCE,     "0: window attention without the MFMA kernels")             \
  X(K_LOSS_PPT,           "USSEG_LOSS_PPT",           INT,     4,     ONCE,     "softmax + loss kernel: pixels per thread")
// clang-format on

enum Knob {
#define X(id, name, kind, def, life, doc) id,
  USSEG_KNOBS(X)
#undef X
};
enum { KNOB_INT, KNOB_PRESENT, KNOB_ONCE, KNOB_PER_CALL };
struct KnobDef { const char* name; int kind; int64_t def; int life; };
constexpr KnobDef kKnobs[] = {
#define X(id, name, kind, def, life, doc) {name, KNOB_##kind, def, KNOB_##life},
  USSEG_KNOBS(X)
#undef X
};

// The value of switch K.  A ONCE switch is a function-local static of its own instantiation: filled at the first use of that switch,
// by one thread (the language's guarantee for local statics), shared by every file that uses it.  Hidden: no exported symbols.
template <Knob K>
__attribute__((visibility("hidden"))) inline int64_t knob() {
  auto read = [] {
    const char* v = getenv(kKnobs[K].name);
    return kKnobs[K].kind == KNOB_PRESENT ? (int64_t)(v != nullptr) : (v ? (int64_t)atoll(v) : kKnobs[K].def);
  };
  if constexpr (kKnobs[K].life == KNOB_PER_CALL) return read();
  else {
    static const int64_t v = read();
    return v;
  }
}
