// What the FP64 matrix-core kernels share (gemm_f64.hip, thc.hip): the accumulator type, the XCD-aware unit id, the unit decode
// and the accumulator store.  Everything here has internal linkage: each translation unit compiles its own copy.
#pragma once
#include "common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

// ---- what the kernels share: unit decode, accumulator store, issue order ------------------------------------------------------------
// XCD-aware unit id: hardware deals consecutive block ids round-robin over 8 XCDs; give each XCD a
// contiguous range of units so that neighbours (which share operand panels) share an L2.  Units past the caller's count are
// the padding of the last round.
__device__ __forceinline__ int64_t xcd_unit(int64_t nunits_pad) {
  const int64_t bid = blockIdx.x;
  const int64_t per_xcd = nunits_pad / 8;
  return (bid % 8) * per_xcd + bid / 8;
}

struct Tile { int tm, tn, slab; };      // slab stays 0 where K is not cut (NN)
struct KRange { int64_t k0, k1; };

// slab-major units, row tile fastest
__device__ __forceinline__ Tile decode_tile(int64_t unit, int ntm, int ntn) {
  return {(int)(unit % ntm), (int)((unit / ntm) % ntn), (int)(unit / ((int64_t)ntm * ntn))};
}

__device__ __forceinline__ KRange slab_range(int slab, int64_t kslab, int64_t K) {
  const int64_t k0 = (int64_t)slab * kslab;
  return {k0, (k0 + kslab < K) ? k0 + kslab : K};
}

}  // namespace

// epilogue: D[row = (lane>>4) + 4r][col = lane&15] per 16x16 accumulator; (ROW0, COL0) is the corner of the wave's NI x NJ
// accumulators, entries past the M x N edge are dropped.  STORE is a statement that sees i, j, r, row and col.  A macro, not a
// function template: through a functor the stores of the NT kernels compiled to another epilogue than the one measured.
#define ISDF_STORE_ACC(NI, NJ, ROW0, COL0, M, N, STORE)                                       \
  _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                            \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                           \
      const int row = ROW0 + i * 16 + (lane >> 4) + 4 * r;                                    \
      if (row >= M) continue;                                                                 \
      _Pragma("unroll") for (int j = 0; j < NJ; ++j) {                                        \
        const int col = COL0 + j * 16 + (lane & 15);                                          \
        if (col >= N) continue;                                                               \
        STORE                                                                                 \
      }                                                                                       \
    }                                                                                         \
  }
