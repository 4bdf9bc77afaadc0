// LadderDeployer._bb_stable's walk (strategies/grid/ladder_deployer.py:42-56)
// on a tile's LDS slots, shared by bb_stable_kernel (bq_impulse.hip) and
// grid_ladder_kernel (bq_ladder.hip): a slot per candle holds the row's width
// (upper - lower) / mid, a bit per slot (a wave ballot per 64 slots) marks the
// rows on which the method returns False (mid <= 0, then width <= 0; a NaN row
// passes both tests), and "all n rows valid" is a popcount of the window's
// mask bits, not a walk.
#pragma once
#include "bq_device.h"

namespace bq {

// a row's width and whether the method returns False on it (:48-53)
__device__ __forceinline__ bool bb_row(double upper, double mid, double lower, double& w) {
  w = (upper - lower) / mid;
  return mid <= 0.0 || w <= 0.0;
}

// candle t's slot: NaN and not bad outside the panel
__device__ __forceinline__ bool bb_slot(const double* __restrict__ up, const double* __restrict__ md,
                                        const double* __restrict__ lw, int t, int T, double& w) {
  w = qnan();
  bool bad = false;
  if (t >= 0 && t < T) {
    const double m = md[t];
    w = (up[t] - lw[t]) / m;
    bad = m <= 0.0 || w <= 0.0;
  }
  return bad;
}

// the window of the n slots ending at slot k (k - (n - 1) >= 1, n <= 64): its
// first slot, and the mask words and bits that hold its rows' flags
struct BbWindow {
  int lo, wl, wh;
  uint64_t lo_mask, hi_mask;
};
__device__ __forceinline__ BbWindow bb_window(int k, int n) {
  BbWindow w;
  w.lo = k - (n - 1);
  w.wl = w.lo / WAVE;
  w.wh = k / WAVE;
  w.hi_mask = ~0ull >> (WAVE - 1 - (k & (WAVE - 1)));   // bits 0 .. k % 64
  w.lo_mask = ~0ull << (w.lo & (WAVE - 1));              // bits lo % 64 .. 63
  return w;
}
// the bad rows among them (at most two mask words). A macro over the kernel's
// own LDS array: as a function taking a pointer the two reads are scheduled
// differently, and bb_stable_kernel's code would no longer be what it was
#define BQ_BB_WINDOW_BAD(sBad, w)                                          \
  ((w).wl == (w).wh ? __popcll((sBad)[(w).wh] & (w).hi_mask & (w).lo_mask) \
                    : __popcll((sBad)[(w).wl] & (w).lo_mask) + __popcll((sBad)[(w).wh] & (w).hi_mask))

// change_pct of the window's first and last widths (:55)
__device__ __forceinline__ double bb_change(double w0, double w1) { return fabs((w1 - w0) / w0) * 100.0; }

}  // namespace bq
