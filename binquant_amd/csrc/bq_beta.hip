// Rolling beta / correlation of each symbol's log returns against the
// benchmark's (BTC), at every timestamp of an index-aligned [S][T] panel.
//
// Restates ContextEvaluator.dynamic_btc_beta_corr
// (producers/context_evaluator.py:154-194): returns = log(c / c.shift(1)) for
// the symbol and for BTC, inner-joined on the index and dropna'd (so the
// series start at candle 1), then with pandas' rolling(window) kernels
// (pandas/core/window/rolling.py cov/corr, pandas 2.3.3):
//   mean_xy, mean_x, mean_y = roll_mean(...)            (same-value rule)
//   cov  = (mean_xy - mean_x * mean_y) * (n / (n - 1))
//   beta = cov / var_y            (var_y == 0 -> NaN: var.replace(0, nan))
//   corr = cov / (var_x * var_y) ** 0.5                 (roll_var, ddof 1)
// NaN where the window is incomplete (t < window). A missing (NaN) or zero
// close drops its pairs as the reference's dropna does: the window is the
// last `window` valid pairs, and a candle without a pair repeats the last
// valid pair's value (beta_gap_row below).
//
// One wave per symbol walks the row in tiles of 256 candles (4 per lane), with
// no cross-wave step: waves of different symbols never wait for each other,
// so one's latency hides behind another's arithmetic (the 256-thread block
// walker this replaces spent most of its time in barriers). Per candle the
// window sums come from tile-local prefix sums (wave DPP scans) in an LDS ring
// of 512 candles: a window sum is one difference, O(1) per candle whatever the
// window. At the end of a tile the lanes holding its last 128 prefixes write
// them back re-based to the next tile's frame (minus the tile total), so the
// prefixes never grow past one tile (no cancellation on long rows) and a read
// needs no frame test. The squares are summed about row-constant references
// (the row's first return) so the variances do not cancel; the means follow
// pandas' roll_mean including its same-value rule (runs of equal values,
// tracked with wave max-scans and a per-tile carry), so constant-return
// windows (a halted symbol: returns exactly 0) give pandas' exact 0
// covariance / NaN correlation. The previous candle of lane 0 and the run /
// total carries come from the previous tile through readlane; the next tile's
// prices are in flight while the current one computes.
#include "bq_rowtile.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// beta_btc_stats_kernel's block: 256 threads, 4 candles per lane; the halo
// holds a whole window of prefixes (the wave kernel shares K and H)
using BC = RowTile<256, 4, 128>;
static_assert(BC::H >= BQ_MAX_WINDOW + 2, "ring shape");

struct BetaArgs {
  const double* close;   // PAIRS: symbol returns
  const double* btc;     // PAIRS: benchmark returns, same row stride
  double* beta;
  double* corr;
  const double* ystat;   // MODE 3: [3][T] benchmark window mean, variance (ddof 1), 1 / variance
  int64_t ld_in, ld_out;
  int T, win;
  double inv_w, inv_w1, bias;   // 1/w, 1/(w-1), w/(w-1)
  int vin, vbtc, vout;   // 16-byte aligned rows: close / btc loads, beta / corr stores
};

// 1 / sqrt(v) for v >= 0 (+inf at 0) with two Newton steps
__device__ __forceinline__ double rsq_nr(double v) {
  const double r0 = __builtin_amdgcn_rsq(v);
  const double h = 0.5 * v;
  double r = r0 * fma(-h * r0, r0, 1.5);
  r = r * fma(-h * r, r, 1.5);
  return v > 0.0 ? r : r0;   // select, not a branch
}

// inclusive wave prefix sum of a double (DPP row scans + readlane row carries)
__device__ __forceinline__ double wave_scan_f64(double x, int lane) {
  x += dpp_f64<DPP_ROW_SHR1>(x);
  x += dpp_f64<DPP_ROW_SHR2>(x);
  x += dpp_f64<DPP_ROW_SHR4>(x);
  x += dpp_f64<DPP_ROW_SHR8>(x);
  const double r0 = readlane_f64(x, 15), r1 = readlane_f64(x, 31), r2 = readlane_f64(x, 47);
  const int row = lane >> 4;
  const double c = row == 0 ? 0.0 : (row == 1 ? r0 : (row == 2 ? r0 + r1 : (r0 + r1) + r2));
  return x + c;
}

// A lane's 4 consecutive candles are two 16-byte accesses where the row allows
// (load_lane; each instruction then fills half of every line it touches
// instead of a quarter; nontemporal loads measured slower here, nontemporal
// stores faster: store_lines, which the wave's lanes all call).
constexpr int BW_TT = WAVE * BC::K;   // candles per tile
constexpr int BW_R = 512;            // ring: a tile plus a halo of up to 256 candles
constexpr int BW_Q = BW_R / BC::K;
static_assert(BW_R >= BW_TT + BC::H && (BW_R & (BW_R - 1)) == 0 && BC::K == 4, "wave ring shape");
// candle index (negative: before the row) -> ring slot, lane-interleaved
__device__ __forceinline__ int wslot(int t) {
  const unsigned p = (unsigned)t & (BW_R - 1);
  return (int)((p & (BC::K - 1)) * BW_Q + (p >> 2));
}
#ifndef BQ_BW_WAVES
#define BQ_BW_WAVES 3   // waves per SIMD the MODE 3 register budget is cut for
#endif

// A row with a candle that lacks a finite return pair (a missing or zero
// close on either side). The reference drops the pairs with a NaN return and
// rolls over the compacted rest: the window at t is the last `win` valid
// pairs however far back they lie, NaN while fewer exist, and NaN while it
// holds a +-inf return (pandas' rolling takes it for a missing observation
// without dropping the pair); a candle without a pair of its own repeats the
// last valid pair's value (the reference's iloc[-1]). The prefix walk lets
// such a pair add nothing, so it is right wherever the last `win` positions
// all hold finite pairs and wrong elsewhere. After the walk the same wave
// passes over the row again, one lane per candle, and recomputes the tiles
// of 64 candles that hold a candle within `win` of a bad pair: each lane
// walks back over the row (L2 hits: the walk has just read it) until it
// holds `win` valid pairs and forms the sums directly about its own pair
// (x0, y0), with the same-value rule where every x / y / x*y of the window
// is equal. The benchmark's window stats of the pre-pass (MODE 3) are not
// read here: they hold the benchmark's own validity, not the pair's.
template <int MODE>
__device__ __forceinline__ void beta_pair(const double* __restrict__ rc, const double* __restrict__ rb, int j,
                                          double& x, double& y) {
  if (MODE == 1) {
    x = rc[j];
    y = rb[j];
  } else {
    x = log_return(rc[j], rc[j - 1]);
    y = MODE >= 2 ? rb[j] : log_return(rb[j], rb[j - 1]);
  }
}

__device__ __forceinline__ bool finite_pair(double x, double y) {
  return fabs(x) <= __DBL_MAX__ && fabs(y) <= __DBL_MAX__;
}

template <int MODE>
__device__ __forceinline__ void beta_gap_row(const BetaArgs& A, const double* __restrict__ rc,
                                             const double* __restrict__ rb, int64_t orow, int win, int lane) {
  constexpr int t_first = MODE == 1 ? 0 : 1;
  const int T = A.T;
  double carb = qnan(), carc = qnan();   // the last valid pair's value before this tile
  bool car_mem = false;                  // ... is the walk's, at t0 - 1 (the tile before was kept)
  int dprev = win;                       // candles from t0 - 1 back to the last bad pair, at most win
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    const bool in = t >= t_first && t < T;
    double x0 = 0.0, y0 = 0.0;
    if (in) beta_pair<MODE>(rc, rb, t, x0, y0);
    const bool have = in && x0 == x0 && y0 == y0;
    // candles since the last bad pair: below win, the window at t holds it
    const unsigned long long le = ~0ull >> (WAVE - 1 - lane);
    const unsigned long long mb = __builtin_amdgcn_ballot_w64(in && !finite_pair(x0, y0)) & le;
    const int d = mb ? lane - (63 - __builtin_clzll(mb)) : lane + 1 + dprev;
    dprev = min(__builtin_amdgcn_readlane(d, WAVE - 1), win);
    if (__builtin_amdgcn_ballot_w64(in && d < win) == 0) {   // the walk's values stand
      car_mem = true;
      continue;
    }
    if (car_mem) {   // t0 - 1 has a pair and a clean window: its value is the last valid pair's
      carb = A.beta ? A.beta[orow + t0 - 1] : qnan();
      carc = A.corr ? A.corr[orow + t0 - 1] : qnan();
      car_mem = false;
    }
    double beta = qnan(), corr = qnan();
    if (have && finite_pair(x0, y0)) {
      const double xy0 = x0 * y0;
      double sx = 0.0, sy = 0.0, sxy = 0.0, su = 0.0, suu = 0.0, sv = 0.0, svv = 0.0;
      bool samex = true, samey = true, samexy = true;
      int n = 0;
      for (int j = t; j >= t_first; --j) {
        double x, y;
        beta_pair<MODE>(rc, rb, j, x, y);
        if (x != x || y != y) continue;    // dropna
        if (!finite_pair(x, y)) break;     // +-inf in the window: NaN
        const double xy = x * y, u = x - x0, v = y - y0;
        sx += x;
        sy += y;
        sxy += xy;
        su += u;
        sv += v;
        suu = fma(u, u, suu);
        svv = fma(v, v, svv);
        samex = samex && x == x0;
        samey = samey && y == y0;
        samexy = samexy && xy == xy0;
        if (++n == win) break;
      }
      if (n == win) {
        const double mx = samex ? x0 : sx * A.inv_w, my = samey ? y0 : sy * A.inv_w;
        const double mxy = samexy ? xy0 : sxy * A.inv_w;
        double vx = samex ? 0.0 : (suu - su * su * A.inv_w) * A.inv_w1;
        double vy = samey ? 0.0 : (svv - sv * sv * A.inv_w) * A.inv_w1;
        vx = vx < 0.0 ? 0.0 : vx;
        vy = vy < 0.0 ? 0.0 : vy;
        const double cov = (mxy - mx * my) * A.bias;
        beta = cov * (vy == 0.0 ? qnan() : rcp_nr(vy));
        corr = cov * rsq_nr(vx * vy);
      }
    }
    // candles without a pair: the nearest lane below that has one, else the carry
    const unsigned long long below = __builtin_amdgcn_ballot_w64(have) & le;
    const int src = below ? 63 - __builtin_clzll(below) : 0;
    const double sb = __shfl(beta, src, WAVE), sc = __shfl(corr, src, WAVE);
    if (!have) {
      beta = below ? sb : carb;
      corr = below ? sc : carc;
    }
    carb = readlane_f64(beta, WAVE - 1);
    carc = readlane_f64(corr, WAVE - 1);
    if (t < T) {
      if (A.beta) A.beta[orow + t] = beta;
      if (A.corr) A.corr[orow + t] = corr;
    }
  }
}

// MODE 0: close / btc prices, returns formed here (first return NaN, first
// full window at t = w). MODE 2: close prices + the benchmark's returns as one
// row shared by every symbol (formed once per launch, not once per wave).
// MODE 1: rows of dropna'd return pairs (bq_join_returns), first full window
// at t = w - 1.
// MODE 3: as MODE 2, and the benchmark's window mean / variance / inverse
// variance at every t are read from A.ystat (beta_btc_stats_kernel, once per
// launch): the wave scans three series (x, x*y, (x - rx)^2) instead of five.
template <int MODE>
__global__ __launch_bounds__(WAVE, MODE == 3 ? BQ_BW_WAVES : 2) void beta_wave_kernel(const BetaArgs A) {
  constexpr bool PAIRS = MODE == 1, BRET = MODE >= 2, YST = MODE == 3;
  constexpr int NS = YST ? 3 : 5;   // x, x*y, (x - rx)^2 [, y, (y - ry)^2]
  __shared__ double sP[NS][BW_R];
  const int lane = threadIdx.x;
  const int64_t sym = blockIdx.x;
  const double* __restrict__ rc = A.close + sym * A.ld_in;
  const double* __restrict__ rb = PAIRS ? A.btc + sym * A.ld_in : A.btc;
  const int T = A.T;
  const int win = __builtin_amdgcn_readfirstlane(A.win);
  // row references of the squared deviations: the first return
  const int t_first = PAIRS ? 0 : 1;
  double rx = 0.0, ry = 0.0;
  if (T > t_first) {
    rx = PAIRS ? rc[0] : log_return(rc[1], rc[0]);
    ry = PAIRS ? rb[0] : (BRET ? rb[1] : log_return(rb[1], rb[0]));
    if (!(fabs(rx) <= __DBL_MAX__)) rx = 0.0;   // any finite reference serves
    if (!(fabs(ry) <= __DBL_MAX__)) ry = 0.0;
  }
  // empty prefixes before the row (the halo of the first tile)
#pragma unroll
  for (int h = 0; h < BC::H; h += WAVE)
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) sP[s2][wslot(h + lane - BC::H)] = 0.0;
  // carries of the previous tile (wave-uniform)
  double cprev = qnan(), bprev = qnan(), xprev = qnan(), yprev = qnan(), xyprev = qnan();
  int carx = -1, cary = -1, carxy = -1;
  const bool vin = A.vin, vbtc = A.vbtc, vout = A.vout;
  double cn[BC::K], bn[BC::K];
  load_lane<BC::K>(rc, BC::K * lane, T, vin, cn);
  load_lane<BC::K>(rb, BC::K * lane, T, vbtc, bn);
  const double wd = (double)win;
  // nonzero once the lane met a candle inside the row without a finite pair:
  // the row is recomputed (beta_gap_row). An int, so that it lives in a VGPR:
  // the walk has scalar registers for nothing more.
  int gap = 0;
  for (int t0 = 0; t0 < T; t0 += BW_TT) {
    const int tb = t0 + BC::K * lane;
    // MODE 3: the benchmark's window stats of this tile (L2 hits: every symbol
    // reads the same rows), issued before the next tile's prefetch so that
    // waiting for them does not wait for it (loads retire in order)
    double ym[BC::K], yv[BC::K], yi[BC::K];
    if (YST) {
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        const bool ok = tb + k < T;
        ym[k] = ok ? A.ystat[tb + k] : 0.0;
        yv[k] = ok ? A.ystat[T + tb + k] : 0.0;
        yi[k] = ok ? A.ystat[2 * T + tb + k] : 0.0;
      }
    }
    double x[BC::K], y[BC::K];
    {
      double c[BC::K], b[BC::K];
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        c[k] = cn[k];
        b[k] = bn[k];
      }
      if (t0 + BW_TT < T) {   // next tile's inputs in flight during this one
        load_lane<BC::K>(rc, tb + BW_TT, T, vin, cn);
        load_lane<BC::K>(rb, tb + BW_TT, T, vbtc, bn);
      }
      double pc = dpp_f64<DPP_WAVE_SHR1>(c[BC::K - 1]), pbt = dpp_f64<DPP_WAVE_SHR1>(b[BC::K - 1]);
      if (lane == 0) {
        pc = cprev;
        pbt = bprev;
      }
      cprev = readlane_f64(c[BC::K - 1], WAVE - 1);
      if (!BRET) bprev = readlane_f64(b[BC::K - 1], WAVE - 1);
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        if (PAIRS) {
          x[k] = c[k];
          y[k] = b[k];
        } else {
          x[k] = log_return(c[k], pc);   // NaN at candle 0 (dropna)
          y[k] = BRET ? b[k] : log_return(b[k], pbt);
        }
        pc = c[k];
        pbt = b[k];
      }
    }
    // per-candle terms (a candle without both returns, finite, adds nothing), their
    // tile-local inclusive prefixes, and the last index where x / y / x*y
    // changed (the same-value rule)
    double q[NS][BC::K];
    int lcx[BC::K], lcy[BC::K], lcxy[BC::K];
    {
      double acc[NS];
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) acc[s2] = 0.0;
      double px = dpp_f64<DPP_WAVE_SHR1>(x[BC::K - 1]), py = dpp_f64<DPP_WAVE_SHR1>(y[BC::K - 1]);
      double pxy = dpp_f64<DPP_WAVE_SHR1>(x[BC::K - 1] * y[BC::K - 1]);
      if (lane == 0) {
        px = xprev;
        py = yprev;
        pxy = xyprev;
      }
      int lx = -1, ly = -1, lxy = -1;
      int bad = 0;
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        const int t = tb + k;
        const double xy = x[k] * y[k];
        // both returns finite: one test of the product (|log return| < 746: it cannot overflow)
        const bool ok = __builtin_isfinite(xy);
        // rows of joined pairs end in NaN padding, which is no gap: there only +-inf
        if (PAIRS ? __builtin_isinf(x[k]) || __builtin_isinf(y[k]) : !ok && (k > 0 || t != 0)) bad = 1;   // candle 0 has no return
        if (ok) {
          const double u = x[k] - rx;
          acc[0] += x[k];
          acc[1] += xy;
          acc[2] = fma(u, u, acc[2]);
          if (!YST) {
            const double v = y[k] - ry;
            acc[3] += y[k];
            acc[4] = fma(v, v, acc[4]);
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) q[s2][k] = acc[s2];
        if (t == 0 || !(x[k] == px)) lx = t;
        if (!YST && (t == 0 || !(y[k] == py))) ly = t;   // MODE 3: the benchmark's own runs are in ystat
        if (t == 0 || !(xy == pxy)) lxy = t;
        lcx[k] = lx;
        lcy[k] = ly;
        lcxy[k] = lxy;
        px = x[k];
        py = y[k];
        pxy = xy;
      }
      if (PAIRS || t0 + BW_TT <= T) {
        gap |= bad;
      } else {   // the ragged last tile: the lanes past T hold padding
#pragma unroll
        for (int k = 0; k < BC::K; ++k)
          if (!__builtin_isfinite(x[k] * y[k]) && tb + k >= t_first && tb + k < T) gap = 1;
      }
      xprev = readlane_f64(x[BC::K - 1], WAVE - 1);
      if (!YST) yprev = readlane_f64(y[BC::K - 1], WAVE - 1);
      xyprev = readlane_f64(x[BC::K - 1] * y[BC::K - 1], WAVE - 1);
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) {
        const double ex = wave_scan_f64(acc[s2], lane) - acc[s2];
#pragma unroll
        for (int k = 0; k < BC::K; ++k) q[s2][k] += ex;
      }
      const int ix = wave_scan_max_dpp(lx + 1, lane) - 1, iy = YST ? -1 : wave_scan_max_dpp(ly + 1, lane) - 1,
                ixy = wave_scan_max_dpp(lxy + 1, lane) - 1;
      const int cx = max(carx, dpp_i32<DPP_WAVE_SHR1>(ix + 1) - 1),
                cy = YST ? -1 : max(cary, dpp_i32<DPP_WAVE_SHR1>(iy + 1) - 1),
                cxy = max(carxy, dpp_i32<DPP_WAVE_SHR1>(ixy + 1) - 1);
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        lcx[k] = max(lcx[k], cx);
        lcy[k] = max(lcy[k], cy);
        lcxy[k] = max(lcxy[k], cxy);
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) sP[s2][wslot(tb + k)] = q[s2][k];
      }
    }
    __syncthreads();   // one wave: orders the ring writes before the reads
    double beta[BC::K], corr[BC::K];
#pragma unroll
    for (int k = 0; k < BC::K; ++k) {
      const int t = tb + k;
      // (computed for every lane, the incomplete windows masked at the end:
      // a ring read before the row start is a zeroed slot)
      // window sums: own prefix minus the prefix at t - win (this tile's frame)
      const int o = wslot(t - win);
      double S[NS];
#pragma unroll
      for (int s2 = 0; s2 < NS; ++s2) S[s2] = q[s2][k] - sP[s2][o];
      // pandas: mean_xy, mean_x, mean_y = roll_mean (same-value rule)
      const bool cx = lcx[k] <= t - win + 1, cxy = lcxy[k] <= t - win + 1;
      const double mx = cx ? x[k] : S[0] * A.inv_w;
      const double mxy = cxy ? x[k] * y[k] : S[1] * A.inv_w;
      // variances about the row references: sum (x - rx)^2 - (sum (x - rx))^2 / w
      const double Su = S[0] - wd * rx;
      double vx = cx ? 0.0 : (S[2] - Su * Su * A.inv_w) * A.inv_w1;
      double my, vy, ivy;
      if (YST) {
        my = ym[k];
        vy = yv[k];
        ivy = yi[k];
      } else {
        const bool cy = lcy[k] <= t - win + 1;
        my = cy ? y[k] : S[3] * A.inv_w;
        const double Sv = S[3] - wd * ry;
        vy = cy ? 0.0 : (S[4] - Sv * Sv * A.inv_w) * A.inv_w1;
        vy = vy < 0.0 ? 0.0 : vy;
        ivy = vy == 0.0 ? qnan() : rcp_nr(vy);
      }
      const double cov = (mxy - mx * my) * A.bias;
      vx = vx < 0.0 ? 0.0 : vx;
      // reciprocal / reciprocal square root with Newton refinement (a few ulps,
      // well inside the 1e-9 bar) instead of IEEE divides: cov / vy, and
      // cov / sqrt(vx vy) (+-inf / NaN when vx vy == 0, as pandas' division)
      const bool full = t >= win - (PAIRS ? 1 : 0);
      beta[k] = full ? cov * ivy : qnan();
      corr[k] = full ? cov * rsq_nr(vx * vy) : qnan();
    }
    const int64_t orow = sym * A.ld_out;
    if (A.beta) store_lines<BC::K>(A.beta + orow, tb, T, vout, beta);
    if (A.corr) store_lines<BC::K>(A.corr + orow, tb, T, vout, corr);
    carx = __builtin_amdgcn_readlane(lcx[BC::K - 1], WAVE - 1);
    cary = __builtin_amdgcn_readlane(lcy[BC::K - 1], WAVE - 1);
    carxy = __builtin_amdgcn_readlane(lcxy[BC::K - 1], WAVE - 1);
    if (t0 + BW_TT >= T) break;
    // the halo of the next tile: this tile's last 128 prefixes in the next
    // tile's frame (held in registers by lanes 32..63)
    double tot[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) tot[s2] = readlane_f64(q[s2][BC::K - 1], WAVE - 1);
    __syncthreads();   // this tile's ring reads are done
    if (BC::K * lane >= BW_TT - BC::H) {
#pragma unroll
      for (int k = 0; k < BC::K; ++k)
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) sP[s2][wslot(tb + k)] = q[s2][k] - tot[s2];
    }
  }
  if (__builtin_amdgcn_ballot_w64(gap != 0) != 0) {   // wave-uniform; never taken on a clean row
    __threadfence();   // the walk's stores of this row land before the ones that replace them
    beta_gap_row<MODE>(A, rc, rb, sym * A.ld_out, win, lane);
  }
}

// The benchmark's rolling(w) mean and variance (ddof 1) of its log returns
// at every t (NaN while t < w; pandas' same-value rule: a constant window has
// the value itself as mean and 0 variance): ystat[0][t], ystat[1][t], and
// 1 / variance (NaN where the variance is 0: beta's var.replace(0, nan))
// in ystat[2][t]. One
// 256-thread workgroup walks the row with the prefix scheme of the main
// kernel. y = returns row (y[0] NaN).
// bp != NULL: y is formed here from the benchmark's prices
// (log_return(bp[t], bp[t-1]), NaN at t = 0) and written to ystat[3][t] for
// the symbol walk, so a call needs no separate returns pass.
__global__ __launch_bounds__(BC::NT) void beta_btc_stats_kernel(const double* __restrict__ y,
                                                               const double* __restrict__ bp, int T, int win,
                                                               double inv_w, double inv_w1, double* ystat) {
  __shared__ double sP[2][BC::R];
  __shared__ double sWt[2][BC::NW];
  __shared__ int sWl[BC::NW];
  __shared__ int sCar;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const auto yv = [&](int t) -> double {
    if (t < 0 || t >= T) return qnan();
    if (bp) return t == 0 ? qnan() : log_return(bp[t], bp[t - 1]);
    return y[t];
  };
  double ry = T > 1 ? yv(1) : 0.0;
  if (!(fabs(ry) <= __DBL_MAX__)) ry = 0.0;
  if (tid < BC::H) sP[0][BC::slot(tid)] = sP[1][BC::slot(tid)] = 0.0;
  if (tid == 0) sCar = -1;
  for (int t0 = 0; t0 < T; t0 += BC::TT) {
    const int tb = t0 + BC::K * tid, pb = BC::H + BC::K * tid;
    double v[BC::K], q[2][BC::K], acc[2] = {0.0, 0.0};
    int lc[BC::K], l = -1;
    double pv = tb >= 1 && tb <= T ? yv(tb - 1) : qnan();
#pragma unroll
    for (int k = 0; k < BC::K; ++k) {
      const int t = tb + k;
      v[k] = yv(t);
      if (bp && t < T) ystat[3 * T + t] = v[k];
      if (fabs(v[k]) <= __DBL_MAX__) {   // a missing or +-inf return adds nothing (beta_gap_row)
        const double d = v[k] - ry;
        acc[0] += v[k];
        acc[1] = fma(d, d, acc[1]);
      }
      q[0][k] = acc[0];
      q[1][k] = acc[1];
      if (t == 0 || !(v[k] == pv)) l = t;
      lc[k] = l;
      pv = v[k];
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const double inc = wave_scan_f64(acc[s2], lane);
      if (lane == WAVE - 1) sWt[s2][w] = inc;
#pragma unroll
      for (int k = 0; k < BC::K; ++k) q[s2][k] += inc - acc[s2];
    }
    const int c = block_excl_max(l, &sCar, sWl, lane, w);   // its barrier also publishes sWt
    double base[2] = {0.0, 0.0};
    for (int u = 0; u < w; ++u) {
      base[0] += sWt[0][u];
      base[1] += sWt[1][u];
    }
#pragma unroll
    for (int k = 0; k < BC::K; ++k) {
      lc[k] = max(lc[k], c);
      q[0][k] += base[0];
      q[1][k] += base[1];
      sP[0][BC::slot(pb + k)] = q[0][k];
      sP[1][BC::slot(pb + k)] = q[1][k];
    }
    __syncthreads();
    const double wd = (double)win;
#pragma unroll
    for (int k = 0; k < BC::K; ++k) {
      const int t = tb + k, o = BC::slot(pb + k - win);
      if (t >= T) continue;
      double m = qnan(), var = qnan();
      if (t >= win) {
        const double Sy = q[0][k] - sP[0][o], Svv = q[1][k] - sP[1][o];
        if (lc[k] <= t - win + 1) {
          m = v[k];
          var = 0.0;
        } else {
          m = div_exact(Sy, wd, inv_w);
          const double Sv = Sy - wd * ry;
          var = (Svv - Sv * Sv * inv_w) * inv_w1;
          var = var < 0.0 ? 0.0 : var;
        }
      }
      ystat[t] = m;
      ystat[T + t] = var;
      ystat[2 * T + t] = var == 0.0 ? qnan() : 1.0 / var;
    }
    if (t0 + BC::TT >= T) break;
    double last[2] = {sP[0][BC::slot(BC::R - 1)], sP[1][BC::slot(BC::R - 1)]};
    __syncthreads();
    if (pb >= BC::TT) {
#pragma unroll
      for (int k = 0; k < BC::K; ++k) {
        sP[0][BC::slot(pb + k - BC::TT)] = q[0][k] - last[0];
        sP[1][BC::slot(pb + k - BC::TT)] = q[1][k] - last[1];
      }
    }
    if (tid == BC::NT - 1) sCar = lc[BC::K - 1];
  }
}

}  // namespace bq

namespace {
int launch_beta(int mode, const double* close, const double* btc_close, int64_t S, int64_t T, int64_t ld_in,
                int32_t window, double* beta, double* corr, int64_t ld_out, void* stream,
                double* ystat = nullptr) {
  using namespace bq;
  if (!close || !btc_close || S < 0 || T < 0 || ld_in < T || ld_out < T || window < 2 ||
      window > BQ_MAX_WINDOW || T > 0x7fffffff || S > 0x7fffffff)
    return BQ_EINVAL;
  if (S == 0 || T == 0 || (!beta && !corr)) return BQ_OK;
  BetaArgs A;
  A.close = close;
  A.btc = btc_close;
  A.beta = beta;
  A.corr = corr;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.win = window;
  A.inv_w = 1.0 / (double)window;
  A.inv_w1 = 1.0 / (double)(window - 1);
  A.bias = (double)window / (double)(window - 1);
  A.ystat = ystat;
  const double* const outs[2] = {beta, corr};
  A.vin = vec_row(close, ld_in);
  A.vbtc = aligned16(mode == 4 ? ystat + 3 * T : btc_close) && (mode != 1 || (ld_in & 1) == 0);
  A.vout = vec_rows(outs, 2, ld_out);
  if (mode == 3 || mode == 4) {   // 4: benchmark prices, its returns formed by the pre-pass into ystat[3]
    hipLaunchKernelGGL(beta_btc_stats_kernel, dim3(1), dim3(BC::NT), 0, (hipStream_t)stream,
                       mode == 3 ? btc_close : nullptr, mode == 4 ? btc_close : nullptr, A.T, window, A.inv_w,
                       A.inv_w1, ystat);
    if (mode == 4) A.btc = ystat + 3 * T;
    hipLaunchKernelGGL(beta_wave_kernel<3>, dim3((unsigned)S), dim3(WAVE), 0, (hipStream_t)stream, A);
  } else if (mode == 1) hipLaunchKernelGGL(beta_wave_kernel<1>, dim3((unsigned)S), dim3(WAVE), 0, (hipStream_t)stream, A);
  else if (mode == 2) hipLaunchKernelGGL(beta_wave_kernel<2>, dim3((unsigned)S), dim3(WAVE), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(beta_wave_kernel<0>, dim3((unsigned)S), dim3(WAVE), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
}  // namespace

extern "C" int bq_beta_corr(const double* close, const double* btc_close, int64_t S, int64_t T, int64_t ld_in,
                            int32_t window, double* beta, double* corr, int64_t ld_out, void* stream) {
  return launch_beta(0, close, btc_close, S, T, ld_in, window, beta, corr, ld_out, stream);
}

extern "C" int bq_beta_corr_bret(const double* close, const double* btc_returns, double* scratch, int64_t S,
                                 int64_t T, int64_t ld_in, int32_t window, double* beta, double* corr, int64_t ld_out,
                                 void* stream) {
  return launch_beta(scratch ? 3 : 2, close, btc_returns, S, T, ld_in, window, beta, corr, ld_out, stream, scratch);
}

extern "C" int bq_beta_corr_ws(const double* close, const double* btc_close, double* scratch, int64_t S, int64_t T,
                               int64_t ld_in, int32_t window, double* beta, double* corr, int64_t ld_out,
                               void* stream) {
  if (!scratch) return BQ_EINVAL;
  return launch_beta(4, close, btc_close, S, T, ld_in, window, beta, corr, ld_out, stream, scratch);
}

extern "C" int bq_beta_corr_pairs(const double* x, const double* y, int64_t S, int64_t T, int64_t ld_in,
                                  int32_t window, double* beta, double* corr, int64_t ld_out, void* stream) {
  return launch_beta(1, x, y, S, T, ld_in, window, beta, corr, ld_out, stream);
}
