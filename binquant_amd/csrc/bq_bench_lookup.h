// Benchmark-frame lookup shared by the kernels that join a panel's candles to
// the benchmark (BTC) frame on open_time: bq_lead.hip (lead_kernel) and
// bq_impulse.hip (impulse_kernel). bench_ts is ascending; a repeated time
// resolves to its LAST row (GradualGainerRetest's dict keeps the later row,
// strategies/gradual_gainer_retest.py:139; RelativeStrengthImpulseRider
// ._btc_return_at scans backwards, strategies/relative_strength_impulse_rider.py
// :74-81; bq_align keeps "last").
#pragma once
#include "bq_device.h"

namespace bq {

// bstep of a benchmark frame: the mean spacing, which is the grid step when
// the grid is regular (0: no guess, always search)
__device__ __forceinline__ int64_t bench_step(const int64_t* __restrict__ bts, int nb, int64_t bt0) {
  return nb > 1 ? (bts[nb - 1] - bt0) / (nb - 1) : 0;
}

// Index of the last benchmark row whose time equals key (-1: none); its close
// is written to b (left untouched without a match). On a regular grid the
// guessed row's time, its successor's and its close are loaded together (one
// dependent round trip after the candle's time); a gap, an irregular grid or
// a repeated time falls back to the guessed-then-binary lower bound.
// nb >= 1, bt0 = bts[0], bstep = bench_step(bts, nb, bt0).
__device__ __forceinline__ int bench_last_match(const int64_t* __restrict__ bts, const double* __restrict__ bclose,
                                                int nb, int64_t key, int64_t bt0, int64_t bstep, double& b) {
  int jg = -1;
  if (bstep > 0 && key >= bt0) {
    const int64_t q = (key - bt0) / bstep;
    jg = q < nb ? (int)q : -1;
  }
  if (jg >= 0) {
    const int64_t tg = bts[jg];
    const int64_t tn = jg + 1 < nb ? bts[jg + 1] : INT64_MAX;
    const double bg = bclose[jg];
    if (tg == key && tn != key) {
      b = bg;
      return jg;
    }
  }
  const int j = lower_bound_guess(bts, nb, key + 1, bt0, bstep) - 1;
  if (j >= 0 && bts[j] == key) {
    b = bclose[j];
    return j;
  }
  return -1;
}

}  // namespace bq
