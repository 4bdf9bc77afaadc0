// Fused market-context partials for gfx950 (BASELINE configs[4], C5):
// _compute_symbol_features at every timestamp of a [S][T] panel under the
// MarketStateStore history cap, reduced straight into the per-timestamp
// breadth partials of _build_context without materialising the six feature
// columns (market_regime/live_market_context_accumulator.py:95-163, 244-297).
//
// bq_market_features + bq_breadth_partial write 48 B of features per candle
// and read 56 B back; the panel context build needs only the [T][10]
// partials (plus, optionally, the features of the last timestamp). Here:
//
// pass 1  context_partials_kernel: one WAVE per symbol (4 symbols per
//         workgroup), tiles of 256 candles (4 per lane). The features are
//         those of bq_market.hip's features_kernel, reorganised for a wave:
//         * scans (double-double prefixes of close and true range, the EMA
//           affine maps, the pandas same-value run starts) are wave scans on
//           DPP with tile carries held in registers — no workgroup barrier;
//         * the history-capped EMA uses the exact window identity
//             y_t = Y_t - a^(M-1) (Y_s - c_s),  s = t - M + 1:
//           long caps (a^(M-1) <= 1e-6: span 50 at M >= 346, the store's
//           400) read D_s = Y_s - c_s from a per-wave fp32 ring in LDS (the
//           last 3 tiles' D, written when s was processed; fp32 moves the
//           term by <= 6e-14 |D|); short caps run a second, lagged EMA chain
//           over c[t - M + 1] (a re-read of the row);
//         * the 4 symbols' contributions at each t are summed in the
//           workgroup in a fixed order, (s0 + s1) + (s2 + s3), through two
//           LDS slots (the second pair's sum written back in place), and
//           written as one group record per t: 4 fp64 sums + the 5 counts
//           packed in 16 bits (34 B per 4 candles).
// pass 2  context_group_reduce_kernel: lane = timestamp, the group records
//         of a chunk of groups summed in a fixed order -> [chunk][T][9]
//         (8 groups' loads in flight per lane before their adds);
// pass 3  context_chunk_reduce_kernel: the chunks in order -> [T][10].
//
// No atomics: the result is bitwise reproducible run to run.
//
// Host side: ctx_args fills what every launch of pass 1 shares (the EMA
// constants and the row load are bq_context.h's, shared with bq_market.hip),
// launch_context<FEAT> picks the instantiation; bq_context_partials and
// context_features (bq_market_features' wave-per-symbol path) call both.
#include "bq_context.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

constexpr int CX_NW = 4;                // waves = symbols per workgroup = per group record
constexpr int CX_NT = CX_NW * WAVE;
constexpr int CX_K = CTX_K;               // candles per lane
constexpr int CX_TT = WAVE * CX_K;      // 256-candle wave tile
constexpr int CX_HS = 20;               // short-window halo (BB 20, ATR 14)
constexpr int CX_RS = CX_HS + CX_TT;    // 276
constexpr int CX_Q = CX_RS / CX_K;
static_assert(CX_HS % CX_K == 0 && CX_RS % CX_K == 0, "ring shape");
// ring position i -> LDS slot, lane-interleaved (the lanes' k-th candles side
// by side: conflict-free; qb = CX_HS + 4 lane is a multiple of 4)
#define CXS(i) ((((i) & (CX_K - 1)) * CX_Q) + ((i) >> 2))
constexpr int CX_ATR = 14;   // live_market_context_accumulator.py:268
constexpr int CX_BB = 20;    // :269-270

// packed group counts: 3 bits per field (<= 4 symbols per group)
constexpr int CNT_VALID = 0, CNT_ADV = 3, CNT_DEC = 6, CNT_A20 = 9, CNT_A50 = 12;

struct CtxArgs {
  const double* h;
  const double* l;
  const double* c;
  int64_t S, ld_in;
  int T, M;
  int vin;
  FeatEma E;           // corr zeroed where the lagged chain is not run
  int lag20, lag50;    // the lagged chain is run where corr >= 1e-15 (below, corr * |Y_s - c_s|
                       // is under 1e-15 of the price move: far inside the 1e-9 bar)
  double* gsum[4];     // group sums [ngrp][ld_g]: return, trend, atr_pct, bb_width
  uint16_t* gcnt;      // packed counts [ngrp][ld_g]
  int64_t ld_g;
  double* last[BQ_NUM_FEATURES];   // optional features at t = T - 1, [S] each
  double* feat[BQ_NUM_FEATURES];   // FEAT: the feature columns [S][ld_f] (NULL = skip)
  int64_t ld_f;
  int vout;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 1 / |b| with the hardware reciprocal + 2 Newton steps (rcp_nr). Measured on
// gfx950 over 4M mantissas x 2^[-60,60] (tools/rcp_probe.hip): 0 steps 4.6e-8
// max relative error (fails the 1e-9 contract), 1 step 2.2e-15, 2 steps the
// correctly rounded reciprocal on every sample — a ratio a * r is then within
// about an ulp of numpy's a / b (not bit for bit: a * RN(1/b) rounds twice).
// One step would be 2.5% faster at the shard (1.70 -> 1.66 ms); kept at two.
__device__ __forceinline__ double cx_rcp(double b) { return rcp_nr(fabs(b)); }
// a / b from r = cx_rcp(b): the sign of a / b and a zero numerator exact
__device__ __forceinline__ double cx_mul_rcp(double a, double b, double r) { return b < 0.0 ? -(a * r) : a * r; }
__device__ __forceinline__ double cx_div(double a, double b) { return cx_mul_rcp(a, b, cx_rcp(b)); }

// DIV: pandas' EMA divide by (old_wt + new_wt) is needed (not exactly 1.0)
// RING: span 50's history term from the D ring (long caps); otherwise the
// lagged chains for every span whose a^(M-1) >= 1e-15 (short caps)
// FEAT: bq_market_features — the six feature columns written (whole-line
// stores of each wave's row) instead of reduced: no group records, no
// workgroup barrier
// MC > 0: the history cap as a compile-time constant (the store's 400 bars)
template <bool DIV, bool RING, bool FEAT = false, int MC = 0>
__global__ __launch_bounds__(CX_NT, 3) void context_partials_kernel(const CtxArgs A) {
  __shared__ double sTr[CX_NW][CX_RS], sC[CX_NW][CX_RS];   // true range / close rings per wave
  __shared__ double sR[2][4][CX_TT];   // reduction slots: 4 sums, index k * 64 + lane
  __shared__ uint16_t sN[2][CX_TT];
  // D ring: 3 tiles. A read at s = t - M + 1 (M <= BQ_MAX_HISTORY + 1 = 513) is
  // overwritten first by candle s + 3 CX_TT > t0 + CX_TT - 1, i.e. after this tile.
  __shared__ float sD[RING ? CX_NW : 1][RING ? 3 * CX_TT : 1];

  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int64_t grp = blockIdx.x;
  const int64_t sym = grp * CX_NW + w;
  const bool live = sym < A.S;                  // wave-uniform
  const int64_t row = live ? sym : A.S - 1;     // idle waves walk a valid row, contribute nothing
  const int T = A.T, M = MC > 0 ? MC : A.M;
  const double* __restrict__ rH = A.h + row * A.ld_in;
  const double* __restrict__ rL = A.l + row * A.ld_in;
  const double* __restrict__ rC = A.c + row * A.ld_in;
  double* __restrict__ trr = sTr[w];
  double* __restrict__ cr = sC[w];
  const bool vin = A.vin != 0;
  const int WB = M < CX_BB ? M : CX_BB;   // Bollinger window under the history cap

  if (lane < CX_HS) {
    trr[CXS(lane)] = 0.0;
    cr[CXS(lane)] = qnan();
  }
  // tile carries (wave-uniform): candle t0 - 1 (and close t0 - 2), run starts, EMA states
  double c1c = qnan(), c2c = qnan(), hc = qnan(), lc = qnan();
  int rcC = -1, rtC = -1;
  double ecar[2] = {0.0, 0.0}, lcar[2] = {0.0, 0.0};
  // the scans' lane-constant powers: A^(4 lane) and the row-carry factor
  double lpow[2], rpow[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    lpow[e] = pow_bits<6>(A.E.apow[e], lane);
    rpow[e] = pow_bits<5>(A.E.apow[e], (lane & 15) + 1);
  }
  wave_sync();

  for (int t0 = 0; t0 < T; t0 += CX_TT) {
    const int tb = t0 + CX_K * lane, qb = CX_HS + CX_K * lane;
    double h[CX_K], l[CX_K], c[CX_K], xl[CX_K];
    load4<double2>(rH, tb, T, vin, h);
    load4<double2>(rL, tb, T, vin, l);
    load4<double2>(rC, tb, T, vin, c);
    if (!RING && (A.lag20 || A.lag50)) {
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {   // lagged closes c[t - M + 1] (0 before the row starts)
        const int s = tb + k - (M - 1);
        xl[k] = (s >= 0 && s < T) ? rC[s] : 0.0;
      }
    }

    double p1 = dpp_f64<DPP_WAVE_SHR1>(c[CX_K - 1]);
    double p2 = dpp_f64<DPP_WAVE_SHR1>(c[CX_K - 2]);
    double ph = dpp_f64<DPP_WAVE_SHR1>(h[CX_K - 1]);
    double pl = dpp_f64<DPP_WAVE_SHR1>(l[CX_K - 1]);
    if (lane == 0) {
      p1 = c1c;
      p2 = c2c;
      ph = hc;
      pl = lc;
    }
    double tr[CX_K];
    int lcc[CX_K], lct[CX_K];
    {
      double pcv = p1, ptr = true_range(ph, pl, p2), cp = p1;
      int rc = -1, rt = -1;
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
        const int t = tb + k;
        tr[k] = true_range(h[k], l[k], cp);
        if (t == 0 || c[k] != pcv) rc = t;
        if (t == 0 || tr[k] != ptr) rt = t;
        lcc[k] = rc;
        lct[k] = rt;
        pcv = c[k];
        ptr = tr[k];
        cp = c[k];
      }
    }
#pragma unroll
    for (int k = 0; k < CX_K; ++k) {
      cr[CXS(qb + k)] = c[k];
      trr[CXS(qb + k)] = tr[k];
    }
    // run starts: exclusive wave max (+1 so DPP's zero fill is the identity) and the tile carry
    {
      const int ic = wave_scan_max_dpp(lcc[CX_K - 1] + 1, lane) - 1;
      const int it = wave_scan_max_dpp(lct[CX_K - 1] + 1, lane) - 1;
      const int a = dpp_i32<DPP_WAVE_SHR1>(ic + 1) - 1, b = dpp_i32<DPP_WAVE_SHR1>(it + 1) - 1;
      const int ec = max(lane == 0 ? -1 : a, rcC), et = max(lane == 0 ? -1 : b, rtC);
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
        lcc[k] = max(lcc[k], ec);
        lct[k] = max(lct[k], et);
      }
    }
    // EMA 20 / 50: full-history Y (candle 0 starts it), an affine wave scan +
    // the exact pandas replay of the lane's 4 steps; for the history cap the
    // lagged chain Y_s at s = t - M + 1 (candle 0 starts it M - 1 candles
    // later) where its weight a^(M-1) matters (host: A.lag*)
    double Y[2][CX_K], D[2][CX_K];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double al = A.E.alpha[e], om = A.E.om[e], dn = A.E.den[e];
      {
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < CX_K; ++k) y = (tb + k == 0) ? c[k] : fma(A.E.lin_a[e], y, A.E.lin_b[e] * c[k]);
        const double inc = wave_scan_affine_dpp_rp(y, A.E.apow[e], rpow[e], lane);
        const double ex = dpp_f64<DPP_WAVE_SHR1>(inc);
        double v = lane == 0 ? ecar[e] : fma(lpow[e], ecar[e], ex);
#pragma unroll
        for (int k = 0; k < CX_K; ++k) {
          const double x = c[k];
          if (tb + k == 0) v = x;
          else if (v != x) v = DIV ? (om * v + al * x) / dn : om * v + al * x;
          Y[e][k] = v;
        }
        ecar[e] = readlane_f64(v, WAVE - 1);
      }
      const bool lag = !RING && (e == 0 ? A.lag20 : A.lag50);
#pragma unroll
      for (int k = 0; k < CX_K; ++k) D[e][k] = 0.0;
      if (lag) {
        const int s0 = tb - (M - 1);
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < CX_K; ++k) y = (s0 + k == 0) ? xl[k] : fma(A.E.lin_a[e], y, A.E.lin_b[e] * xl[k]);
        const double inc = wave_scan_affine_dpp_rp(y, A.E.apow[e], rpow[e], lane);
        const double ex = dpp_f64<DPP_WAVE_SHR1>(inc);
        double v = lane == 0 ? lcar[e] : fma(lpow[e], lcar[e], ex);
#pragma unroll
        for (int k = 0; k < CX_K; ++k) {
          const int s = s0 + k;
          const double x = xl[k];
          if (s == 0) v = x;
          else if (s > 0 && v != x) v = DIV ? (om * v + al * x) / dn : om * v + al * x;
          D[e][k] = v - x;
        }
        lcar[e] = readlane_f64(v, WAVE - 1);
      }
    }
    if (RING) {
      float* dr = sD[w];
      const int dslot = ((t0 / CX_TT) % 3) * CX_TT;
#pragma unroll
      for (int k = 0; k < CX_K; ++k) dr[dslot + CX_K * lane + k] = (float)(Y[1][k] - c[k]);
    }
    wave_sync();   // the rings (close, true range) of every lane are visible
    if (RING) {
      const float* dr = sD[w];
      int r = ((t0 / CX_TT) % 3) * CX_TT + CX_K * lane - (M - 1);
      r += r < 0 ? 3 * CX_TT : 0;
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
        const int q = r + k >= 3 * CX_TT ? r + k - 3 * CX_TT : r + k;
        D[1][k] = (double)dr[q];
      }
    }

    // ---- features (_compute_symbol_features, :244-297) ------------------------
    // ATR = TR.rolling(14, min_periods=1).mean(), BB = rolling(20, min_periods=1)
    // mean / std(ddof=0) over the history cap: sliding window sums per lane
    // (the BB sums about a lane-local reference, no cancellation); windows
    // still short of their length (the row's first 19 candles) re-sum
    // directly; pandas' constant-window rule from the run starts.
    double atr[CX_K], mid[CX_K], sd[CX_K];
    if (tb >= CX_BB - 1 && WB == CX_BB) {   // every candle of the lane has full windows
      {
        double a[CX_ATR - 1];
#pragma unroll
        for (int i = 0; i < CX_ATR - 1; ++i) a[i] = trr[CXS(qb - (CX_ATR - 1) + i)];
        double Sx = 0.0;
#pragma unroll
        for (int i = 0; i < CX_ATR - 1; ++i) Sx += a[i];
#pragma unroll
        for (int k = 0; k < CX_K; ++k) {
          Sx = k == 0 ? Sx + tr[0] : (Sx + tr[k]) - a[k - 1];
          atr[k] = div_count(Sx < 0.0 ? 0.0 : Sx, (double)CX_ATR, 1.0 / CX_ATR);
        }
      }
      {
        const double r = c[0];
        double d0[CX_K - 1];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < CX_BB - 1; ++i) {
          const double d = cr[CXS(qb - (CX_BB - 1) + i)] - r;
          if (i < CX_K - 1) d0[i] = d;
          s1 += d;
          s2 = fma(d, d, s2);
        }
#pragma unroll
        for (int k = 0; k < CX_K; ++k) {
          const double dn = c[k] - r;
          if (k == 0) {
            s1 += dn;
            s2 = fma(dn, dn, s2);
          } else {
            const double dol = d0[k - 1];
            s1 = (s1 + dn) - dol;
            s2 = fma(-dol, dol, fma(dn, dn, s2));
          }
          const double m1 = s1 * (1.0 / CX_BB);
          const double var = fma(-m1, s1, s2) * (1.0 / CX_BB);
          mid[k] = r + m1;
          sd[k] = sqrt_nr(var > 0.0 ? var : 0.0);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
        const int t = tb + k, q = qb + k;
        const int n = min(t + 1, M);
        const int ma = min(CX_ATR, n), mb = min(WB, n);
        double Sx = 0.0;
        for (int i = q - ma + 1; i <= q; ++i) Sx += trr[CXS(i)];
        atr[k] = (Sx < 0.0 ? 0.0 : Sx) / (double)ma;
        double m = 0.0;
        for (int i = q - mb + 1; i <= q; ++i) m += cr[CXS(i)];
        m = m / (double)mb;
        double acc = 0.0;
        for (int i = q - mb + 1; i <= q; ++i) {
          const double d = cr[CXS(i)] - m;
          acc = fma(d, d, acc);
        }
        mid[k] = m;
        sd[k] = sqrt(acc / (double)mb);
      }
    }
    double fr[CX_K], fe20[CX_K], fe50[CX_K], ftr[CX_K], fap[CX_K], fbw[CX_K];
    // the closes' reciprocals, each shared by candle k's ATR ratio and candle
    // k + 1's return (5 per lane instead of 8: the same r, the same bits)
    double rc[CX_K + 1];
    rc[0] = cx_rcp(p1);
#pragma unroll
    for (int k = 0; k < CX_K; ++k) rc[k + 1] = cx_rcp(c[k]);
#pragma unroll
    for (int k = 0; k < CX_K; ++k) {
      const int t = tb + k;
      const int n = min(t + 1, M);
      if (n < 2) {   // history.empty or len < 2 -> None (:248-249)
        fr[k] = fe20[k] = fe50[k] = ftr[k] = fap[k] = fbw[k] = qnan();
        continue;
      }
      const double cl = c[k];
      const double prev = k > 0 ? c[k - 1] : p1;
      double e20 = Y[0][k], e50 = Y[1][k];
      if (t + 1 > M) {   // the history window starts at s = t - M + 1 > 0
        e20 = e20 - A.E.corr[0] * D[0][k];
        e50 = e50 - A.E.corr[1] * D[1][k];
      }
      const double a = lct[k] <= t - min(CX_ATR, n) + 1 ? tr[k] : atr[k];
      double m = mid[k], s = sd[k];
      if (lcc[k] <= t - min(WB, n) + 1) {
        m = cl;
        s = 0.0;
      }
      const double up = m + (2.0 * s), lo = m - (2.0 * s);
      fr[k] = prev == 0.0 ? 0.0 : cx_mul_rcp(cl - prev, prev, rc[k]);   // safe_pct (shared/utils.py:20-23)
      fe20[k] = e20;
      fe50[k] = e50;
      ftr[k] = e50 != 0.0 ? cx_div(e20 - e50, e50 < 0.0 ? -e50 : e50) : 0.0;
      fap[k] = cl != 0.0 ? cx_mul_rcp(a, cl, rc[k + 1]) : 0.0;
      fbw[k] = m != 0.0 ? cx_div(up - lo, m < 0.0 ? -m : m) : 0.0;
    }
    if constexpr (FEAT) {
      if (live) {   // wave-uniform: store_lines exchanges across the wave
        const int64_t orow = sym * A.ld_f;
        const bool vo = A.vout != 0, whole = t0 + CX_TT <= T;
        const double* const cols[BQ_NUM_FEATURES] = {fr, fe20, fe50, ftr, fap, fbw};
#pragma unroll
        for (int f = 0; f < BQ_NUM_FEATURES; ++f)
          if (A.feat[f]) {
            double v[CX_K];
#pragma unroll
            for (int k = 0; k < CX_K; ++k) v[k] = cols[f][k];
            store_lines<CX_K>(A.feat[f] + orow, tb, T, vo, v, whole);
          }
      }
    } else {
    // the last timestamp's feature row, when asked (the context's symbol_features)
    if (live && tb <= T - 1 && T - 1 < tb + CX_K) {
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
        if (tb + k != T - 1) continue;
        const double v[BQ_NUM_FEATURES] = {fr[k], fe20[k], fe50[k], ftr[k], fap[k], fbw[k]};
#pragma unroll
        for (int f = 0; f < BQ_NUM_FEATURES; ++f)
          if (A.last[f]) A.last[f][sym] = v[f];
      }
    }

    // ---- this symbol's contributions, then the group's (fixed order) --------
    double cs[4][CX_K];
    unsigned cn[CX_K];
#pragma unroll
    for (int k = 0; k < CX_K; ++k) {
      const double r = fr[k];
      const bool ok = live && tb + k < T && r == r;   // no features at t: nothing counted
      cn[k] = ok ? ((1u << CNT_VALID) | ((r > 0.0 ? 1u : 0u) << CNT_ADV) | ((r < 0.0 ? 1u : 0u) << CNT_DEC) |
                    ((c[k] > fe20[k] ? 1u : 0u) << CNT_A20) | ((c[k] > fe50[k] ? 1u : 0u) << CNT_A50))
                 : 0u;
      cs[0][k] = ok ? r : 0.0;
      cs[1][k] = ok ? ftr[k] : 0.0;
      cs[2][k] = ok ? fap[k] : 0.0;
      cs[3][k] = ok ? fbw[k] : 0.0;
    }
    if (w & 1) {   // waves 1, 3 -> slots 0, 1
      const int sl = w >> 1;
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
#pragma unroll
        for (int f = 0; f < 4; ++f) sR[sl][f][k * WAVE + lane] = cs[f][k];
        sN[sl][k * WAVE + lane] = (uint16_t)cn[k];
      }
    }
    __syncthreads();
    if (!(w & 1)) {   // wave 0: s0 + s1, wave 2: s2 + s3
      const int sl = w >> 1;
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
#pragma unroll
        for (int f = 0; f < 4; ++f) cs[f][k] = cs[f][k] + sR[sl][f][k * WAVE + lane];
        cn[k] += sN[sl][k * WAVE + lane];
      }
      if (w == 2) {
#pragma unroll
        for (int k = 0; k < CX_K; ++k) {
#pragma unroll
          for (int f = 0; f < 4; ++f) sR[1][f][k * WAVE + lane] = cs[f][k];
          sN[1][k * WAVE + lane] = (uint16_t)cn[k];
        }
      }
    }
    __syncthreads();
    if (w == 0) {   // (s0 + s1) + (s2 + s3) -> the group record at t
#pragma unroll
      for (int k = 0; k < CX_K; ++k) {
#pragma unroll
        for (int f = 0; f < 4; ++f) cs[f][k] = cs[f][k] + sR[1][f][k * WAVE + lane];
        cn[k] += sN[1][k * WAVE + lane];
      }
      const int64_t orow = grp * A.ld_g;
#pragma unroll
      for (int f = 0; f < 4; ++f) store_lines<CX_K>(A.gsum[f] + orow, tb, T, true, cs[f]);
      uint16_t* gc = A.gcnt + orow;
      if (tb + CX_K <= T) {
        const uint64_t packed = (uint64_t)cn[0] | ((uint64_t)cn[1] << 16) | ((uint64_t)cn[2] << 32) |
                                ((uint64_t)cn[3] << 48);
        __builtin_nontemporal_store(packed, reinterpret_cast<uint64_t*>(gc + tb));
      } else {
#pragma unroll
        for (int k = 0; k < CX_K; ++k)
          if (tb + k < T) gc[tb + k] = (uint16_t)cn[k];
      }
    }
    }   // !FEAT

    if (t0 + CX_TT >= T) break;
    wave_sync();   // every lane's reads of this tile's rings are done
    if (lane < CX_HS) {   // short halos
      const int src = CX_TT + lane;
      trr[CXS(lane)] = trr[CXS(src)];
      cr[CXS(lane)] = cr[CXS(src)];
    }
    wave_sync();
    c1c = readlane_f64(c[CX_K - 1], WAVE - 1);
    c2c = readlane_f64(c[CX_K - 2], WAVE - 1);
    hc = readlane_f64(h[CX_K - 1], WAVE - 1);
    lc = readlane_f64(l[CX_K - 1], WAVE - 1);
    rcC = __builtin_amdgcn_readlane(lcc[CX_K - 1], WAVE - 1);
    rtC = __builtin_amdgcn_readlane(lct[CX_K - 1], WAVE - 1);
  }
}

// ---- pass 2: group records -> chunk partials ------------------------------------
constexpr int GR_TW = 64;   // timestamps per workgroup (lane = t)
constexpr int GR_NW = 4;
constexpr int GR_U = 8;    // groups in flight per lane
constexpr int CX_NSUM = 9;  // the first 9 partial columns

struct GroupReduceArgs {
  const double* gsum[4];
  const uint16_t* gcnt;
  int64_t ngrp, ld_g, per_chunk;
  int T;
  double* chunk;   // [nchunk][T][9]
};

__global__ __launch_bounds__(GR_TW * GR_NW) void context_group_reduce_kernel(const GroupReduceArgs A) {
  __shared__ double sAcc[GR_NW][CX_NSUM][GR_TW + 1];
  const int lane = threadIdx.x & (WAVE - 1), u = threadIdx.x / WAVE;
  const int t = blockIdx.x * GR_TW + lane;
  const int64_t g0 = (int64_t)blockIdx.y * A.per_chunk;
  const int64_t g1 = min(A.ngrp, g0 + A.per_chunk);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int n[5] = {0, 0, 0, 0, 0};
  auto add = [&](const double (&v)[4], unsigned c) {
#pragma unroll
    for (int f = 0; f < 4; ++f) s[f] += v[f];
    n[0] += (c >> CNT_VALID) & 7u;
    n[1] += (c >> CNT_ADV) & 7u;
    n[2] += (c >> CNT_DEC) & 7u;
    n[3] += (c >> CNT_A20) & 7u;
    n[4] += (c >> CNT_A50) & 7u;
  };
  if (t < A.T) {
    // ascending, fixed per wave; GR_U groups' loads issued before their adds
    // (a load-add loop waits one memory round trip per group)
    int64_t g = g0 + u;
    for (; g + (GR_U - 1) * GR_NW < g1; g += GR_U * GR_NW) {
      double v[GR_U][4];
      unsigned c[GR_U];
#pragma unroll
      for (int j = 0; j < GR_U; ++j) {
        const int64_t o = (g + j * GR_NW) * A.ld_g + t;
#pragma unroll
        for (int f = 0; f < 4; ++f) v[j][f] = A.gsum[f][o];
        c[j] = A.gcnt[o];
      }
#pragma unroll
      for (int j = 0; j < GR_U; ++j) add(v[j], c[j]);
    }
    for (; g < g1; g += GR_NW) {
      const int64_t o = g * A.ld_g + t;
      double v[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) v[f] = A.gsum[f][o];
      add(v, A.gcnt[o]);
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) sAcc[u][i][lane] = (double)n[i];
#pragma unroll
  for (int f = 0; f < 4; ++f) sAcc[u][5 + f][lane] = s[f];
  __syncthreads();
  if (u == 0 && t < A.T) {
    double acc[CX_NSUM];
#pragma unroll
    for (int i = 0; i < CX_NSUM; ++i) acc[i] = sAcc[0][i][lane];
    for (int v = 1; v < GR_NW; ++v)
#pragma unroll
      for (int i = 0; i < CX_NSUM; ++i) acc[i] += sAcc[v][i][lane];
    double* o = A.chunk + ((int64_t)blockIdx.y * A.T + t) * CX_NSUM;
#pragma unroll
    for (int i = 0; i < CX_NSUM; ++i) o[i] = acc[i];
  }
}

// ---- pass 3: chunk partials -> [T][10] ---------------------------------------------
__global__ __launch_bounds__(256) void context_chunk_reduce_kernel(const double* __restrict__ chunk, int nchunk, int T,
                                                                   double* __restrict__ partial) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  double acc[CX_NSUM];
#pragma unroll
  for (int i = 0; i < CX_NSUM; ++i) acc[i] = 0.0;
  for (int j = 0; j < nchunk; ++j) {
    const double* c = chunk + ((int64_t)j * T + t) * CX_NSUM;
#pragma unroll
    for (int i = 0; i < CX_NSUM; ++i) acc[i] += c[i];
  }
  double* o = partial + (int64_t)t * BQ_NUM_PARTIALS;
#pragma unroll
  for (int i = 0; i < CX_NSUM; ++i) o[i] = acc[i];
  o[BQ_P_RESERVED] = 0.0;
}

// ---- workspace layout ---------------------------------------------------------------
struct CtxLayout {
  int64_t ngrp, ld_g, nchunk, per_chunk;
  size_t off_sum[4], off_cnt, off_chunk, bytes;
};

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static CtxLayout ctx_layout(int64_t S, int64_t T) {
  CtxLayout L;
  L.ngrp = (S + CX_NW - 1) / CX_NW;
  L.ld_g = (T + 63) & ~(int64_t)63;
  // enough pass-2 workgroups to fill the chip: ~2048 (t-block, chunk) pairs
  const int64_t tblocks = (T + GR_TW - 1) / GR_TW;
  int64_t nch = (2048 + tblocks - 1) / (tblocks > 0 ? tblocks : 1);
  nch = nch < 1 ? 1 : nch;
  const int64_t maxch = (L.ngrp + 3) / 4;   // at least ~4 groups per chunk
  if (nch > maxch) nch = maxch < 1 ? 1 : maxch;
  L.per_chunk = (L.ngrp + nch - 1) / nch;
  L.nchunk = (L.ngrp + L.per_chunk - 1) / L.per_chunk;
  size_t o = 0;
  for (int f = 0; f < 4; ++f) {
    L.off_sum[f] = o;
    o = align256(o + (size_t)L.ngrp * L.ld_g * sizeof(double));
  }
  L.off_cnt = o;
  o = align256(o + (size_t)L.ngrp * L.ld_g * sizeof(uint16_t));
  L.off_chunk = o;
  o = align256(o + (size_t)L.nchunk * T * CX_NSUM * sizeof(double));
  L.bytes = o;
  return L;
}

// the part of CtxArgs every launch shares: inputs, strides, the vector flag and
// the EMA constants with the history-cap correction factors
static CtxArgs ctx_args(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, int max_bars) {
  CtxArgs A;
  memset(&A, 0, sizeof(A));
  A.h = hlc[0];
  A.l = hlc[1];
  A.c = hlc[2];
  A.S = S;
  A.ld_in = ld_in;
  A.T = (int)T;
  A.M = max_bars;
  A.vin = vec_rows(hlc, 3, ld_in);
  A.E = feat_ema_consts(max_bars);
  A.lag20 = A.E.corr[0] >= 1e-15;
  A.lag50 = A.E.corr[1] >= 1e-15;
  if (!A.lag20) A.E.corr[0] = 0.0;
  if (!A.lag50) A.E.corr[1] = 0.0;
  return A;
}

template <bool FEAT, bool DIV>
static void launch_context_div(const CtxArgs& A, unsigned ngrp, int max_bars, hipStream_t st) {
  // the D ring (fp32) where span 50's term is small: a^(M-1) <= 1e-6 (M >= 346 at
  // span 50), so D's fp32 rounding moves the EMA by <= 6e-14 |D|; span 20's term is
  // then below 1e-15 and skipped
  const bool ring = A.E.corr[1] <= 1e-6 && !A.lag20;
  const dim3 grid(ngrp), block(CX_NT);
  if (!FEAT && ring && max_bars == 400)   // MarketStateStore's default cap, the partials path only
    hipLaunchKernelGGL((context_partials_kernel<DIV, true, false, 400>), grid, block, 0, st, A);
  else if (ring) hipLaunchKernelGGL((context_partials_kernel<DIV, true, FEAT>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((context_partials_kernel<DIV, false, FEAT>), grid, block, 0, st, A);
}

// pass 1 for the partials (FEAT = false) or the feature columns (FEAT = true)
template <bool FEAT>
static void launch_context(const CtxArgs& A, unsigned ngrp, int max_bars, hipStream_t st) {
  if (A.E.den[0] != 1.0 || A.E.den[1] != 1.0) launch_context_div<FEAT, true>(A, ngrp, max_bars, st);
  else launch_context_div<FEAT, false>(A, ngrp, max_bars, st);
}

// bq_market_features through context_partials_kernel<..., FEAT> (bq_market.hip
// calls this): the same per-wave feature computation, the columns written
int context_features(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, int32_t max_bars,
                     double* const* feat, int64_t ld_out, hipStream_t st) {
  CtxArgs A = ctx_args(hlc, S, T, ld_in, max_bars);
  for (int f = 0; f < BQ_NUM_FEATURES; ++f) A.feat[f] = feat[f];
  A.ld_f = ld_out;
  A.vout = vec_rows(feat, BQ_NUM_FEATURES, ld_out);
  launch_context<true>(A, (unsigned)((S + CX_NW - 1) / CX_NW), max_bars, st);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // namespace bq

extern "C" {

size_t bq_context_workspace_bytes(int64_t S, int64_t T) {
  if (S <= 0 || T <= 0) return 0;
  return bq::ctx_layout(S, T).bytes;
}

int bq_context_partials(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, int32_t max_bars,
                        void* workspace, size_t workspace_bytes, double* partial, double* const* last_feat,
                        void* stream) {
  using namespace bq;
  if (!hlc || !hlc[0] || !hlc[1] || !hlc[2] || !partial || S < 0 || T < 0 || ld_in < T || max_bars < 15 ||
      max_bars > BQ_MAX_HISTORY + 1 || T > (int64_t)0x7fffffff - CX_TT || S > (int64_t)0x7fffffff * CX_NW)
    return BQ_EINVAL;
  if (S == 0 || T == 0) {
    if (T > 0 && hipMemsetAsync(partial, 0, (size_t)T * BQ_NUM_PARTIALS * sizeof(double), (hipStream_t)stream) != hipSuccess)
      return BQ_EHIP;
    return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
  }
  const CtxLayout L = ctx_layout(S, T);
  if (!workspace || workspace_bytes < L.bytes || (((uintptr_t)workspace) & 255u)) return BQ_EINVAL;
  CtxArgs A = ctx_args(hlc, S, T, ld_in, max_bars);
  char* ws = (char*)workspace;
  for (int f = 0; f < 4; ++f) A.gsum[f] = (double*)(ws + L.off_sum[f]);
  A.gcnt = (uint16_t*)(ws + L.off_cnt);
  A.ld_g = L.ld_g;
  for (int f = 0; f < BQ_NUM_FEATURES; ++f) A.last[f] = last_feat ? last_feat[f] : nullptr;
  hipStream_t st = (hipStream_t)stream;
  launch_context<false>(A, (unsigned)L.ngrp, max_bars, st);
  GroupReduceArgs G;
  for (int f = 0; f < 4; ++f) G.gsum[f] = A.gsum[f];
  G.gcnt = A.gcnt;
  G.ngrp = L.ngrp;
  G.ld_g = L.ld_g;
  G.per_chunk = L.per_chunk;
  G.T = (int)T;
  G.chunk = (double*)(ws + L.off_chunk);
  hipLaunchKernelGGL(context_group_reduce_kernel, dim3((unsigned)((T + GR_TW - 1) / GR_TW), (unsigned)L.nchunk),
                     dim3(GR_TW * GR_NW), 0, st, G);
  hipLaunchKernelGGL(context_chunk_reduce_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st,
                     (const double*)G.chunk, (int)L.nchunk, (int)T, partial);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // extern "C"
