// The pieces of a wave's sort-and-pick order statistics shared by the tile
// rank kernel (bq_rolling.hip) and the RS-reversal replay (bq_rsreversal.hip):
// order-preserving u64 keys with NaN last, the lane ^ d move of a bitonic
// network, the wave's XOR prefix and the r-th set bit of a multi-word mask.
// Every helper is __forceinline__: a kernel built on them carries the same
// instructions as with the definitions in its own file. Internal to the library.
#pragma once
#include <stdint.h>

#include "bq_device.h"

namespace bq {

__device__ __forceinline__ unsigned long long okey_nan_last(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) x = 0.0;   // -0.0 and +0.0 compare equal
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double okey_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}

// value of lane ^ ld (ld a power of two, a compile-time constant once the
// sort's loops are unrolled): DPP quad permutes for 1 and 2, ds_swizzle's
// xor mode for 4..16 (no address operand), ds_bpermute only across halves
__device__ __forceinline__ unsigned lane_xor(unsigned v, int ld) {
  switch (ld) {
    case 1: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // [1,0,3,2]
    case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // [2,3,0,1]
    case 4: return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (4 << 10));
    case 8: return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (8 << 10));
    case 16: return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (16 << 10));
    default: return __shfl_xor(v, ld, WAVE);
  }
}

// Inclusive XOR prefix of a u32 over the wave (DPP rows + readlane row
// totals; bound_ctrl's 0 is XOR's identity).
__device__ __forceinline__ unsigned wave_scan_xor(unsigned x, int lane) {
  x ^= (unsigned)dpp_i32<DPP_ROW_SHR1>((int)x);
  x ^= (unsigned)dpp_i32<DPP_ROW_SHR2>((int)x);
  x ^= (unsigned)dpp_i32<DPP_ROW_SHR4>((int)x);
  x ^= (unsigned)dpp_i32<DPP_ROW_SHR8>((int)x);
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)x, 15);
  const unsigned r1 = r0 ^ (unsigned)__builtin_amdgcn_readlane((int)x, 31);
  const unsigned r2 = r1 ^ (unsigned)__builtin_amdgcn_readlane((int)x, 47);
  const int row = lane >> 4;
  return x ^ (row == 0 ? 0u : (row == 1 ? r0 : (row == 2 ? r1 : r2)));
}

// index of the r-th (0-based) set bit of the NW-word mask M (r < popcount(M)):
// the word by running popcounts, then a 16/8/4/2/1 popcount bisection in it;
// selects only (no divergent branches)
template <int NW>
__device__ __forceinline__ int select_bit(const unsigned (&M)[NW], int r) {
  unsigned word = 0;
  int base = 0;
  bool found = false;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int c = __popc(M[q]);
    const bool here = !found && r < c;
    word = here ? M[q] : word;
    base = here ? 32 * q : base;
    r = (!found && !here) ? r - c : r;
    found = found || here;
  }
  int p = 0;
#pragma unroll
  for (int h = 16; h >= 1; h >>= 1) {
    const int c = __popc(word & ((1u << h) - 1u));
    const bool up = r >= c;
    r = up ? r - c : r;
    p = up ? p + h : p;
    word = up ? word >> h : word;
  }
  return base + p;
}

}  // namespace bq
