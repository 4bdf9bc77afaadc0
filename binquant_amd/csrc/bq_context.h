// What the market-context kernels share (bq_market.hip, bq_context.hip,
// bq_fresh.hip): the EMA 20 / 50 constants of _compute_symbol_features, the
// 16-byte alignment rule of the vector paths and the four-candle row load.
// Internal to the library.
#pragma once
#include <stdint.h>

#include "bq_device.h"

namespace bq {

constexpr int CTX_K = 4;   // candles per lane in all three files

// pandas ewm(span, adjust=False) for spans 20 / 50
// (market_regime/live_market_context_accumulator.py:266-267)
struct FeatEma {
  double alpha[2], om[2], den[2], lin_a[2], lin_b[2];
  double apow[2][8];   // lin_a^(4 * 2^j)
  double corr[2];      // lin_a^(max_bars - 1): weight of the candle that left the history window
};

inline FeatEma feat_ema_consts(int max_bars) {
  FeatEma E;
  const double spans[2] = {20.0, 50.0};
  for (int e = 0; e < 2; ++e) {
    const double al = 1.0 / (1.0 + (spans[e] - 1.0) / 2.0);
    E.alpha[e] = al;
    E.om[e] = 1.0 - al;
    E.den[e] = E.om[e] + al;
    E.lin_a[e] = E.om[e] / E.den[e];
    E.lin_b[e] = al / E.den[e];
    double ak = 1.0;
    for (int k = 0; k < CTX_K; ++k) ak *= E.lin_a[e];
    for (int j = 0; j < 8; ++j) {
      E.apow[e][j] = ak;
      ak *= ak;
    }
    double cp = 1.0;
    for (int k = 0; k < max_bars - 1; ++k) cp *= E.lin_a[e];
    E.corr[e] = cp;
  }
  return E;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// the 16-byte vector path over n rows-of-doubles arrays of one stride: an even
// stride and every given (non-null) base aligned
inline int vec_rows(const double* const* p, int n, int64_t ld) {
  bool v = (ld % 2) == 0;
  for (int i = 0; i < n; ++i) v = v && (!p[i] || aligned16(p[i]));
  return v;
}

// candles tb .. tb + 3 of a row; past T, 0.0 or (NAN_PAD) NaN. V2: the 16-byte
// vector type of the aligned path (each kernel keeps the one it was compiled
// with); the pad is a template flag because a pad argument moved
// panel_compact_kernel's instruction schedule
template <typename V2, bool NAN_PAD = false>
__device__ __forceinline__ void load4(const double* __restrict__ row, int tb, int T, bool vec, double (&x)[CTX_K]) {
  if (vec && tb + CTX_K <= T) {
    const V2* p = reinterpret_cast<const V2*>(row + tb);
    const V2 a = p[0], b = p[1];
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  } else {
#pragma unroll
    for (int k = 0; k < CTX_K; ++k) x[k] = (tb + k < T) ? row[tb + k] : (NAN_PAD ? qnan() : 0.0);
  }
}

}  // namespace bq
