// Per-symbol regime panel (gfx950): the symbol_features entry every candle of
// a [S][T_out] panel would have read from the market context it saw — has
// features, micro regime and transition with their strengths, the EMA flags,
// relative strength vs BTC and three gathered features — in one streaming pass
// over the six feature columns and the close of a panel context build.
//
//   RegimeTransitionDetector.annotate_context
//     (market_regime/regime_transitions.py:25-43): a symbol's transition is
//     taken against its entry in the immediately previous stored context
//     (_get_previous_context, live_market_context_accumulator.py:86-93), not
//     against its own latest earlier regime; absent from that context: none.
//   _annotate_symbol_regime / _symbol_transition_event (:162-232, :251-277):
//     the arithmetic below, restated from bq_regime.hip's micro_regime_kernel
//     (moving that kernel's code into a shared header changed its device code,
//     so it stays where it is; tests/test_regime_panel_gpu.py holds the two
//     bit-equal). Reference operation order, true fp64 divisions, Python's
//     min / max tie rules; the file is built with -ffp-contract=off.
//   _build_context (:108-123): relative_strength_vs_btc = return_pct - BTC's,
//     0.0 for BTC itself and for everybody when BTC has no features.
//
// The regime at (s, j) depends on that column's features only and the
// transition on the regime and strength at the predecessor column, so the
// pass is time-parallel. One wave per 256-candle tile of a row, four
// consecutive candles per lane (bq_context.h's load4 and alignment rule).
// Where the tile sees its own columns in order (at[t] == t, prev[t] == t - 1:
// tested once per tile, wave-uniformly) each column's regime is computed once
// and the predecessor comes from the neighbouring candle: in the lane's own
// registers, from the lane below (__shfl_up), and for the tile's first candle
// from one recomputed halo column. Any other tile gathers column at[t] and
// recomputes the regime at prev[t]. No atomics, no LDS, no barrier.
#include "bq_context.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

__device__ __forceinline__ double clampd(double x, double lo = -1.0, double hi = 1.0) {
  // shared/utils.py:12-13: max(low, min(high, value))
  const double m = x < hi ? x : hi;   // Python min(high, x): x if x < high else high
  return m > lo ? m : lo;              // Python max(low, m): m if m > low else low
}
// shared/utils.py:16-17 max(0.0, value): value if value > 0.0 else 0.0 (-0.0 -> 0.0)
__device__ __forceinline__ double nneg(double x) { return x > 0.0 ? x : 0.0; }
__device__ __forceinline__ double pmin(double a, double b) { return b < a ? b : a; }   // Python min(a, b)

// the micro regime of one symbol in one context (:162-214); st: its strength
__device__ __forceinline__ int micro_classify(double ts, bool above20, bool above50, double r, double bw, double ap,
                                              double ret, double& st) {
  const double a20 = above20 ? 1.0 : 0.0, a50 = above50 ? 1.0 : 0.0;
  const double up = clampd(0.45 * nneg(ts * 30.0) + 0.2 * a20 + 0.15 * a50 + 0.2 * nneg(r * 20.0), 0.0, 1.0);
  const double down = clampd(0.45 * nneg(-ts * 30.0) + 0.2 * (1.0 - a20) + 0.15 * (1.0 - a50) + 0.2 * nneg(-r * 20.0),
                             0.0, 1.0);
  const double rng = clampd(0.38 * (1.0 - pmin(fabs(ts) * 30.0, 1.0)) + 0.34 * (1.0 - pmin(bw / 0.08, 1.0)) +
                                0.28 * (1.0 - pmin(ap / 0.04, 1.0)),
                            0.0, 1.0);
  const double vol = clampd(0.55 * pmin(ap / 0.05, 1.0) + 0.45 * pmin(bw / 0.12, 1.0), 0.0, 1.0);
  // Python max(a, b, c, d): the first of the largest
  st = up;
  if (down > st) st = down;
  if (rng > st) st = rng;
  if (vol > st) st = vol;
  int reg = BQ_MICRO_TRANSITIONAL;
  if (vol >= 0.72 && fabs(ret) >= 0.015) reg = BQ_MICRO_VOLATILE;
  else if (up >= 0.52 && up >= down + 0.1) reg = BQ_MICRO_TREND_UP;
  else if (down >= 0.52 && down >= up + 0.1) reg = BQ_MICRO_TREND_DOWN;
  else if (rng >= 0.5) reg = BQ_MICRO_RANGE;
  return reg;
}

// the transition out of the predecessor's regime pr (negative: the symbol had
// no entry in the previous context) with strength ps into reg (:216-232,
// :251-277): the event, -1 for None, and its strength
__device__ __forceinline__ int micro_transition(int pr, double ps, int reg, double st, double& tst) {
  int tr = -1;
  tst = 0.0;
  if (pr >= 0 && pr != reg) {
    if (reg == BQ_MICRO_VOLATILE) tr = BQ_MT_VOLATILITY_EXPANSION;
    else if ((pr == BQ_MICRO_RANGE || pr == BQ_MICRO_TRANSITIONAL) && reg == BQ_MICRO_TREND_UP) tr = BQ_MT_BREAKOUT_UP;
    else if ((pr == BQ_MICRO_RANGE || pr == BQ_MICRO_TRANSITIONAL) && reg == BQ_MICRO_TREND_DOWN) tr = BQ_MT_BREAKDOWN;
    else if (pr == BQ_MICRO_TREND_DOWN && reg == BQ_MICRO_TREND_UP) tr = BQ_MT_RECOVERY;
    else if (pr == BQ_MICRO_TREND_UP && reg == BQ_MICRO_RANGE) tr = BQ_MT_MEAN_REVERSION;
    else if (reg == BQ_MICRO_TREND_UP) tr = BQ_MT_ENTERED_TREND_UP;
    else if (reg == BQ_MICRO_TREND_DOWN) tr = BQ_MT_ENTERED_TREND_DOWN;
    else if (reg == BQ_MICRO_RANGE) tr = BQ_MT_ENTERED_RANGE;
    else tr = BQ_MT_ENTERED_TRANSITIONAL;
    tst = clampd(st + fabs(st - ps) - 0.25, 0.0, 1.0);
  }
  return tr;
}

constexpr int RP_K = CTX_K;
constexpr int RP_TT = WAVE * RP_K;   // candles per wave tile
constexpr int RP_NW = 4;             // waves (consecutive tiles) per workgroup
constexpr int RP_NONE = 255;         // _lib.MR_NONE

struct RegimePanelArgs {
  const double* f[BQ_NUM_FEATURES];
  const double* c;
  const int32_t* rank;
  const int32_t* at;
  const int32_t* prev;
  const double* btc;
  const int8_t* seed_regime;
  const double* seed_strength;
  uint8_t* o8[BQ_RP_NUM_U8];
  double* o64[BQ_RP_NUM_F64];
  int64_t S, ld_f, ld_c, ld_r, ld_o8, ld_o64, btc_row, waves;
  int Tc, T, ntiles;
  int vec_in, vec_rank, vec_o8, vec_o64;
  int need_reg, need_prev;
};

// one symbol's entry in one context column: its six features, the close and BTC's return there
struct RpCol {
  double v[BQ_NUM_FEATURES];
  double cl, rs;
  bool has, a20, a50;
};

// relative_strength_vs_btc and the EMA flags (:117-123, :295-296) of a loaded column
__device__ __forceinline__ void rp_derive(RpCol& C, double btc, bool is_btc) {
  C.rs = (btc != btc || is_btc) ? 0.0 : C.v[BQ_F_RETURN] - btc;
  C.a20 = C.cl > C.v[BQ_F_EMA20];
  C.a50 = C.cl > C.v[BQ_F_EMA50];
}

__device__ __forceinline__ int rp_classify(const RpCol& C, double& st) {
  return micro_classify(C.v[BQ_F_TREND], C.a20, C.a50, C.rs, C.v[BQ_F_BB_WIDTH], C.v[BQ_F_ATR_PCT], C.v[BQ_F_RETURN],
                        st);
}

// symbol s's entry in context column j (0 <= j < Tc), gathered: through rank
// where the build was a fresh one (bq_breadth.hip's convention: features at
// k = rank[s][j], none where k < 1), else at j itself (none at j = 0)
__device__ __forceinline__ void rp_gather(const RegimePanelArgs& A, int64_t s, int j, RpCol& C) {
  int k = j;
  if (A.rank) k = A.rank[s * A.ld_r + j];
  C.has = k >= 1 && k < A.Tc;
  if (!C.has) return;
#pragma unroll
  for (int i = 0; i < BQ_NUM_FEATURES; ++i) C.v[i] = A.f[i][s * A.ld_f + k];
  C.cl = A.c[s * A.ld_c + k];
  rp_derive(C, A.btc[j], s == A.btc_row);
}

// the predecessor's (regime or -1, strength) at context column p
__device__ __forceinline__ void rp_pred(const RegimePanelArgs& A, int64_t s, int p, int& pr, double& ps) {
  pr = -1;
  ps = 0.0;
  if (p == -2) {   // the seed: the last snapshot of the chunk before
    if (A.seed_regime) pr = A.seed_regime[s];
    if (A.seed_strength) ps = A.seed_strength[s];
  } else if (p >= 0 && p < A.Tc) {
    RpCol P;
    rp_gather(A, s, p, P);
    if (P.has) pr = rp_classify(P, ps);
  }
}

// a lane's four results into the requested columns
struct RpOut {
  uint8_t b[BQ_RP_NUM_U8][RP_K];
  double d[BQ_RP_NUM_F64][RP_K];
};

__device__ __forceinline__ void rp_none(RpOut& O, int k) {
  O.b[BQ_RP_OK][k] = 0;
  O.b[BQ_RP_MICRO_REGIME][k] = RP_NONE;
  O.b[BQ_RP_MICRO_TRANSITION][k] = RP_NONE;
  O.b[BQ_RP_ABOVE_EMA20][k] = 0;
  O.b[BQ_RP_ABOVE_EMA50][k] = 0;
#pragma unroll
  for (int i = 0; i < BQ_RP_NUM_F64; ++i) O.d[i][k] = qnan();
}

__device__ __forceinline__ void rp_fill(RpOut& O, int k, const RpCol& C, int reg, double st, int tr, double tst) {
  O.b[BQ_RP_OK][k] = 1;
  O.b[BQ_RP_MICRO_REGIME][k] = (uint8_t)reg;
  O.b[BQ_RP_MICRO_TRANSITION][k] = tr >= 0 ? (uint8_t)tr : (uint8_t)RP_NONE;
  O.b[BQ_RP_ABOVE_EMA20][k] = C.a20 ? 1 : 0;
  O.b[BQ_RP_ABOVE_EMA50][k] = C.a50 ? 1 : 0;
  O.d[BQ_RP_RS_VS_BTC][k] = C.rs;
  O.d[BQ_RP_REGIME_STRENGTH][k] = st;
  O.d[BQ_RP_TRANSITION_STRENGTH][k] = tst;
  O.d[BQ_RP_TREND_SCORE][k] = C.v[BQ_F_TREND];
  O.d[BQ_RP_ATR_PCT][k] = C.v[BQ_F_ATR_PCT];
  O.d[BQ_RP_BB_WIDTH][k] = C.v[BQ_F_BB_WIDTH];
}

// candles tb .. tb + 3 (< T) of row s: one 4-byte store per flag column and
// two 16-byte stores per value column where the rows allow
__device__ __forceinline__ void rp_store(const RegimePanelArgs& A, int64_t s, int tb, const RpOut& O) {
  const bool whole = tb + RP_K <= A.T;
#pragma unroll
  for (int i = 0; i < BQ_RP_NUM_U8; ++i) {
    if (!A.o8[i]) continue;
    uint8_t* __restrict__ row = A.o8[i] + s * A.ld_o8;
    if (A.vec_o8 && whole) {
      *reinterpret_cast<uint32_t*>(row + tb) = (uint32_t)O.b[i][0] | ((uint32_t)O.b[i][1] << 8) |
                                               ((uint32_t)O.b[i][2] << 16) | ((uint32_t)O.b[i][3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < RP_K; ++k)
        if (tb + k < A.T) row[tb + k] = O.b[i][k];
    }
  }
#pragma unroll
  for (int i = 0; i < BQ_RP_NUM_F64; ++i) {
    if (!A.o64[i]) continue;
    double* __restrict__ row = A.o64[i] + s * A.ld_o64;
    if (A.vec_o64 && whole) {
      dbl2* p = reinterpret_cast<dbl2*>(row + tb);
      p[0] = dbl2{O.d[i][0], O.d[i][1]};
      p[1] = dbl2{O.d[i][2], O.d[i][3]};
    } else {
#pragma unroll
      for (int k = 0; k < RP_K; ++k)
        if (tb + k < A.T) row[tb + k] = O.d[i][k];
    }
  }
}

typedef int rp_int4 __attribute__((ext_vector_type(4)));

// a tile that sees its own columns in order: column t for candle t, column
// t - 1 its predecessor. Every candle of the tile lies below min(T, Tc)
template <bool FRESH>
__device__ __forceinline__ void rp_tile_fast(const RegimePanelArgs& A, int64_t s, int t0, int lane) {
  const int tb = t0 + RP_K * lane;
  const bool is_btc = s == A.btc_row;
  RpCol C[RP_K];
  if constexpr (!FRESH) {
    double x[BQ_NUM_FEATURES + 1][RP_K];
#pragma unroll
    for (int i = 0; i < BQ_NUM_FEATURES; ++i) load4<dbl2, true>(A.f[i] + s * A.ld_f, tb, A.T, A.vec_in != 0, x[i]);
    load4<dbl2, true>(A.c + s * A.ld_c, tb, A.T, A.vec_in != 0, x[BQ_NUM_FEATURES]);
#pragma unroll
    for (int k = 0; k < RP_K; ++k) {
#pragma unroll
      for (int i = 0; i < BQ_NUM_FEATURES; ++i) C[k].v[i] = x[i][k];
      C[k].cl = x[BQ_NUM_FEATURES][k];
      C[k].has = tb + k >= 1 && tb + k < A.T;
      rp_derive(C[k], tb + k < A.T ? A.btc[tb + k] : qnan(), is_btc);
    }
  } else {
    int rk[RP_K];
    const int32_t* __restrict__ rr = A.rank + s * A.ld_r;
    if (A.vec_rank && tb + RP_K <= A.T) {
      const rp_int4 q = *reinterpret_cast<const rp_int4*>(rr + tb);
      rk[0] = q.x, rk[1] = q.y, rk[2] = q.z, rk[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < RP_K; ++k) rk[k] = tb + k < A.T ? rr[tb + k] : -1;
    }
#pragma unroll
    for (int k = 0; k < RP_K; ++k) {
      C[k].has = rk[k] >= 1 && rk[k] < A.Tc;
      const int kk = C[k].has ? rk[k] : 0;   // column 0 exists (Tc >= 1 here): a harmless read
#pragma unroll
      for (int i = 0; i < BQ_NUM_FEATURES; ++i) C[k].v[i] = A.f[i][s * A.ld_f + kk];
      C[k].cl = A.c[s * A.ld_c + kk];
      rp_derive(C[k], tb + k < A.T ? A.btc[tb + k] : qnan(), is_btc);
    }
  }
  int reg[RP_K], pr = -1;
  double st[RP_K], ps = 0.0;
  if (A.need_reg) {
#pragma unroll
    for (int k = 0; k < RP_K; ++k) {
      reg[k] = rp_classify(C[k], st[k]);
      if (!C[k].has) reg[k] = -1;
    }
    if (A.need_prev) {
      // the candle before the lane's first: the lane below's last, or the halo column
      pr = __shfl_up(reg[RP_K - 1], 1, WAVE);
      ps = __shfl_up(st[RP_K - 1], 1, WAVE);
      if (lane == 0) rp_pred(A, s, t0 - 1, pr, ps);   // t0 = 0: column -1, no predecessor
    }
  }
  RpOut O;
#pragma unroll
  for (int k = 0; k < RP_K; ++k) {
    if (C[k].has) {
      int tr = -1;
      double tst = 0.0, stk = 0.0;
      int rg = RP_NONE;
      if (A.need_reg) {
        rg = reg[k];
        stk = st[k];
        if (A.need_prev) tr = micro_transition(pr, ps, rg, stk, tst);
      }
      rp_fill(O, k, C[k], rg, stk, tr, tst);
    } else {
      rp_none(O, k);
    }
    if (A.need_reg) {
      pr = reg[k];
      ps = st[k];
    }
  }
  rp_store(A, s, tb, O);
}

// any other tile: candle t reads context column at[t] (none below 0) and the
// regime at prev[t] (-1: none; -2: the seed)
__device__ __forceinline__ void rp_tile_generic(const RegimePanelArgs& A, int64_t s, int t0, int lane) {
  const int tb = t0 + RP_K * lane;
  RpOut O;
#pragma unroll
  for (int k = 0; k < RP_K; ++k) {
    rp_none(O, k);
    const int t = tb + k;
    if (t >= A.T) continue;
    const int j = A.at[t];
    if (j < 0 || j >= A.Tc) continue;
    RpCol C;
    rp_gather(A, s, j, C);
    if (!C.has) continue;
    int rg = RP_NONE, tr = -1;
    double st = 0.0, tst = 0.0;
    if (A.need_reg) {
      rg = rp_classify(C, st);
      if (A.need_prev) {
        int pr;
        double ps;
        rp_pred(A, s, A.prev[t], pr, ps);
        tr = micro_transition(pr, ps, rg, st, tst);
      }
    }
    rp_fill(O, k, C, rg, st, tr, tst);
  }
  rp_store(A, s, tb, O);
}

__global__ __launch_bounds__(RP_NW* WAVE) void symbol_regime_panel_kernel(const RegimePanelArgs A) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int64_t gw = (int64_t)blockIdx.x * RP_NW + w;
  if (gw >= A.waves) return;   // wave-uniform; the kernel has no barrier
  const int64_t s = gw / A.ntiles;
  const int t0 = (int)(gw - s * A.ntiles) * RP_TT;
  const int tb = t0 + RP_K * lane;
  bool mine = true;
#pragma unroll
  for (int k = 0; k < RP_K; ++k) {
    const int t = tb + k;
    if (t < A.T) mine = mine && t < A.Tc && A.at[t] == t && A.prev[t] == t - 1;
  }
  if (__all(mine)) {
    if (A.rank) rp_tile_fast<true>(A, s, t0, lane);
    else rp_tile_fast<false>(A, s, t0, lane);
  } else {
    rp_tile_generic(A, s, t0, lane);
  }
}

}  // namespace bq

extern "C" {

int bq_symbol_regime_panel(const double* const* feat, int64_t ld_f, const double* close, int64_t ld_c,
                           const int32_t* rank, int64_t ld_r, int64_t S, int64_t Tc, const int32_t* at,
                           const int32_t* prev, int64_t T_out, const double* btc_return, int64_t btc_row,
                           const int8_t* seed_regime, const double* seed_strength, uint8_t* const* out_u8,
                           int64_t ld_u8, double* const* out_f64, int64_t ld_f64, void* stream) {
  using namespace bq;
  constexpr int64_t cap = (int64_t)0x7fffffff - RP_TT;
  if (!feat || !close || !at || !prev || !btc_return || !out_u8 || !out_f64 || S < 0 || Tc < 0 || T_out < 0 ||
      Tc > cap || T_out > cap || ld_f < Tc || ld_c < Tc || (rank && ld_r < Tc) || ld_u8 < T_out || ld_f64 < T_out ||
      btc_row < -1 || btc_row >= (S > 0 ? S : 1) || S > (int64_t)0x7fffffff)
    return BQ_EINVAL;
  for (int i = 0; i < BQ_NUM_FEATURES; ++i)
    if (!feat[i]) return BQ_EINVAL;
  const int64_t ntiles = (T_out + RP_TT - 1) / RP_TT;
  if (S * ntiles > (int64_t)0x7fffffff) return BQ_EINVAL;
  if (S == 0 || T_out == 0) return BQ_OK;
  RegimePanelArgs A;
  memset(&A, 0, sizeof(A));
  for (int i = 0; i < BQ_NUM_FEATURES; ++i) A.f[i] = feat[i];
  A.c = close;
  A.rank = rank;
  A.at = at;
  A.prev = prev;
  A.btc = btc_return;
  A.seed_regime = seed_regime;
  A.seed_strength = seed_strength;
  bool any = false;
  for (int i = 0; i < BQ_RP_NUM_U8; ++i) {
    A.o8[i] = out_u8[i];
    any = any || A.o8[i];
  }
  for (int i = 0; i < BQ_RP_NUM_F64; ++i) {
    A.o64[i] = out_f64[i];
    any = any || A.o64[i];
  }
  if (!any) return BQ_OK;
  A.S = S;
  A.ld_f = ld_f;
  A.ld_c = ld_c;
  A.ld_r = ld_r;
  A.ld_o8 = ld_u8;
  A.ld_o64 = ld_f64;
  A.btc_row = btc_row;
  A.Tc = (int)Tc;
  A.T = (int)T_out;
  A.ntiles = (int)ntiles;
  A.waves = S * ntiles;
  A.vec_in = vec_rows(feat, BQ_NUM_FEATURES, ld_f) && vec_row(close, ld_c);
  A.vec_rank = rank && (ld_r % 4) == 0 && aligned16(rank);
  A.vec_o8 = vec_bytes(out_u8, BQ_RP_NUM_U8, ld_u8);
  A.vec_o64 = vec_rows(out_f64, BQ_RP_NUM_F64, ld_f64);
  A.need_prev = A.o8[BQ_RP_MICRO_TRANSITION] || A.o64[BQ_RP_TRANSITION_STRENGTH];
  A.need_reg = A.need_prev || A.o8[BQ_RP_MICRO_REGIME] || A.o64[BQ_RP_REGIME_STRENGTH];
  const unsigned blocks = (unsigned)((A.waves + RP_NW - 1) / RP_NW);
  hipLaunchKernelGGL(symbol_regime_panel_kernel, dim3(blocks), dim3(RP_NW * WAVE), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // extern "C"
