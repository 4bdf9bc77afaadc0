// What the market-context kernels share (bq_market.hip, bq_context.hip,
// bq_fresh.hip): the EMA 20 / 50 constants of _compute_symbol_features, the
// vector type of the four-candle row load (the load itself and the 16-byte
// alignment rule of the vector paths: bq_rowtile.h).
// Internal to the library.
#pragma once
#include <stdint.h>

#include "bq_rowtile.h"

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

// candles tb .. tb + 3 of a row (load_lane); past T, 0.0 or (NAN_PAD) NaN. V2:
// the 16-byte vector type of the aligned path (each kernel keeps the one it
// was compiled with); the pad is a template flag because a pad argument moved
// panel_compact_kernel's instruction schedule
template <typename V2, bool NAN_PAD = false>
__device__ __forceinline__ void load4(const double* __restrict__ row, int tb, int T, bool vec, double (&x)[CTX_K]) {
  load_lane<CTX_K, NAN_PAD, V2>(row, tb, T, vec, x);
}

}  // namespace bq
