// The workgroup-per-row mapping shared by the strategy, signal, panel and
// context kernels: one workgroup walks a row in tiles, each lane holding K
// consecutive candles, the series that windows read in an LDS ring with a halo
// of H candles (the previous tile's last ones) in front of the tile. Every
// helper is __forceinline__: a kernel built on them compiles to the code of
// the hand-written copies they replaced (`make isa-digest`).
// Internal to the library.
#pragma once
#include <stdint.h>

#include "bq_device.h"

namespace bq {

// NT threads, K candles per lane, halo H. Ring position p (0 .. H - 1 the
// halo, H + K * tid + k a lane's k-th candle) lives at slot(p): lane-interleaved,
// so the lanes' k-th candles sit side by side (in the natural layout they are
// K apart: multi-way bank conflicts on every access).
template <int NT_, int K_, int H_>
struct RowTile {
  static constexpr int NT = NT_, K = K_, H = H_;
  static constexpr int NW = NT / WAVE;
  static constexpr int TT = NT * K;   // candles per tile
  static constexpr int R = H + TT;    // ring positions
  static constexpr int Q = R / K;
  static_assert(NT % WAVE == 0 && (K & (K - 1)) == 0 && R % K == 0 && H % K == 0, "ring shape");
  // p / K as a shift: ring positions are never negative
  static __device__ __forceinline__ int slot(int p) { return (p & (K - 1)) * Q + (p >> __builtin_ctz(K)); }
};

// A lane's K candles tb .. tb + K - 1 of a row: 16-byte loads where the row
// allows (vec: an even stride and an aligned base, wave-uniform) and the lane
// lies inside the row, else element-wise with NaN (NAN_PAD) or 0.0 past T.
// V2: the 16-byte vector type of the aligned path; the context kernels keep
// HIP's double2 (bq_context.h).
template <int K, bool NAN_PAD = true, typename V2 = dbl2>
__device__ __forceinline__ void load_lane(const double* __restrict__ row, int tb, int T, bool vec, double (&x)[K]) {
  if (vec && tb + K <= T) {
    const V2* p = reinterpret_cast<const V2*>(row + tb);
#pragma unroll
    for (int j = 0; j < K / 2; ++j) {
      const V2 a = p[j];
      x[2 * j] = a.x;
      x[2 * j + 1] = a.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = tb + k < T ? row[tb + k] : (NAN_PAD ? qnan() : 0.0);
  }
}

// A lane's 4 flags of consecutive candles: one 4-byte store when the row
// allows (vec4: a stride that is a multiple of 4 and an aligned base)
template <int K>
__device__ __forceinline__ void put_bytes(uint8_t* __restrict__ row, int tb, int T, bool vec4, const bool (&b)[K]) {
  static_assert(K == 4, "put_bytes: one dword of flags per lane");
  if (vec4 && tb + K <= T) {
    const uint32_t w = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    *reinterpret_cast<uint32_t*>(row + tb) = w;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (tb + k < T) row[tb + k] = b[k] ? 1 : 0;
  }
}

// Exclusive block max of a per-lane int >= -1 (wave DPP scan, the waves'
// totals through sW[NW]) combined with the tile carry `*carry` — read after
// the barrier: the previous tile's last thread writes it after that tile's
// final barrier, so a read before this one would race. Every thread of the
// block calls it (one barrier).
__device__ __forceinline__ int block_excl_max(int v, const int* carry, int* sW, int lane, int w) {
  const int inc = wave_scan_max_dpp(v + 1, lane) - 1;   // +1: DPP's zero fill is the identity
  if (lane == WAVE - 1) sW[w] = inc;
  const int lpre = dpp_i32<DPP_WAVE_SHR1>(inc + 1) - 1;   // lane 0 -> -1
  __syncthreads();
  int c = max(*carry, lpre);
  for (int u = 0; u < w; ++u) c = max(c, sW[u]);
  return c;
}

// ---- which rows take the vector paths (host side of a launch) ----------------
__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// one array of rows: an aligned base and an even stride (also called in the
// panel kernels, whose jobs each bring their own arrays)
__host__ __device__ __forceinline__ bool vec_row(const void* p, int64_t ld) { return aligned16(p) && (ld % 2) == 0; }

// the 16-byte vector path over n rows-of-doubles arrays of one stride: an even
// stride and every given (non-null) base aligned
inline int vec_rows(const double* const* p, int n, int64_t ld) {
  bool v = (ld % 2) == 0;
  for (int i = 0; i < n; ++i) v = v && (!p[i] || aligned16(p[i]));
  return v;
}

// its twin for the flag columns' 4-byte stores: a stride that is a multiple of
// 4 and every given (non-null) base 4-byte aligned
inline int vec_bytes(const uint8_t* const* p, int n, int64_t ld) {
  bool v = (ld % 4) == 0;
  for (int i = 0; i < n; ++i) v = v && (!p[i] || (((uintptr_t)p[i]) & 3u) == 0);
  return v;
}

}  // namespace bq
