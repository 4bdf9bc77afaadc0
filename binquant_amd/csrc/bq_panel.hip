// Time-parallel ("panel mode") rolling sums / means and ewm (gfx950) for the
// strategy pipelines of SURVEY §8a a17-a19 on a [S][T] panel, at the
// north_star tolerance (1e-9 of pandas) instead of the bit-exact replay:
//
//   x.shift(shift).rolling(window, min_periods).sum() / .mean()
//       strategies/failed_spike_fade.py:260-318, liquidation_sweep_pump.py:220
//   x.ewm(alpha, adjust=False, min_periods).mean()
//       strategies/liquidation_sweep_pump.py:215-217, 252-253, 265-266
//
// The exact replays of bq_rolling.hip are lane = symbol, sequential along T:
// 12.5k symbols are 196 waves per series for 1 024 SIMDs, each a 2 000-step
// dependent chain. Here one 256-thread workgroup per (row, series) walks the
// row in tiles of 2 048 candles (8 per lane, 64-byte loads, the next tile in
// flight), the values in an LDS ring with a 128-candle halo (window + shift
// <= 128), lane-interleaved (conflict-free):
//
// * sum / mean: one sliding walk per lane (window + 8 ring reads per 8
//   outputs), NaN skipped with pandas' observation count and min_periods, the
//   same-value rule (the window's values all equal -> the value itself, x
//   nobs for sums) from the run starts of the row (a block max-scan of the
//   last index where the value changed) — a window holding a NaN compares its
//   values directly — and calc_mean's sign rule from sliding negative counts;
// * ewm: an associative scan of the affine maps y -> la y + lb x (wave
//   shuffles, LDS across waves, a tile carry), then each lane replays its 8
//   steps with pandas' update (weighted = old_wt w + alpha x, / (old_wt +
//   alpha), skipped when w == x). A row with a missing or infinite value
//   continues serially from the first tile that holds one with pandas' own
//   recursion (gap decay of the old weight, the observation count, a late
//   first observation): exact, and only such rows pay for it.
//
// Values agree with pandas to rounding (the replay's Kahan / online sums are
// not reproduced bit for bit); bq_rolling_batch keeps the replays for
// bq_roll_job.panel == 0 (the live path and every bit-exact test).
#include "bq_panel.h"

#include "bq_rowtile.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// 256 threads, 8 candles per lane (tiles of 2048, ring of 2176 in 8 planes of
// 272); halo 128 >= window + shift. The jobs of a batch each bring their own
// arrays, so the vector-path test (vec_row) runs in the kernel.
using PN = RowTile<256, 8, 128>;

// ---- sum / mean -----------------------------------------------------------------------
__global__ __launch_bounds__(PN::NT) void panel_window_kernel(const PanelBatch B) {
  __shared__ double sX[PN::R];
  __shared__ int sL[PN::R];   // run start (last index where the value changed) per ring position
  __shared__ int sW[PN::NW];
  __shared__ int sCar;
  const PanelJob& A = B.j[blockIdx.y];
  const int64_t row = blockIdx.x;
  if (row >= A.rows) return;   // the job's own row count (a benchmark row): uniform per block
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const double* __restrict__ x = A.x + row * A.ld_in;
  double* __restrict__ out = A.out + row * A.ld_out;
  const int T = B.T, win = A.win, sh = A.shift, minp = A.minp;
  const bool mean = A.mode == BQ_ROLL_MEAN;
  const bool vin = vec_row(A.x, A.ld_in), vout = vec_row(A.out, A.ld_out);
  if (tid < PN::H) {   // before the row: missing values
    sX[PN::slot(tid)] = qnan();
    sL[PN::slot(tid)] = -1;
  }
  if (tid == 0) sCar = -1;
  double nx[PN::K];
  load_lane<PN::K>(x, PN::K * tid, T, vin, nx);
  for (int t0 = 0; t0 < T; t0 += PN::TT) {
    const int tb = t0 + PN::K * tid, pb = PN::H + PN::K * tid;
    double c[PN::K];
#pragma unroll
    for (int k = 0; k < PN::K; ++k) c[k] = win_val(nx[k]);   // +-inf is missing (pandas' window ops)
    const double pc0 = tb >= 1 && tb <= T ? win_val(x[tb - 1]) : qnan();
    if (t0 + PN::TT < T) load_lane<PN::K>(x, tb + PN::TT, T, vin, nx);
    // run starts of the values (NaN counts as a change)
    int lcl[PN::K];
    {
      double pv = pc0;
      int run = -1;
#pragma unroll
      for (int k = 0; k < PN::K; ++k) {
        if (tb + k == 0 || !(c[k] == pv)) run = tb + k;
        lcl[k] = run;
        pv = c[k];
      }
      const int carry = block_excl_max(lcl[PN::K - 1], &sCar, sW, lane, w);
#pragma unroll
      for (int k = 0; k < PN::K; ++k) lcl[k] = max(lcl[k], carry);
    }
#pragma unroll
    for (int k = 0; k < PN::K; ++k) {
      sX[PN::slot(pb + k)] = c[k];
      sL[PN::slot(pb + k)] = lcl[k];
    }
    __syncthreads();
    // window of output t = tb + k: ring positions [pb + k - sh - win + 1, pb + k - sh]
    double s = 0.0;
    int nobs = 0, neg = 0;
    const int e0 = pb - sh;   // position of the entering value of output k = 0
    for (int j = 1 - win; j <= 0; ++j) {
      const double v = sX[PN::slot(e0 + j)];
      const bool ok = v == v;
      s += ok ? v : 0.0;
      nobs += ok;
      neg += ok && signbit(v);
    }
    double res[PN::K];
#pragma unroll
    for (int k = 0; k < PN::K; ++k) {
      const int e = e0 + k;   // entering position
      if (k > 0) {
        const double vi = sX[PN::slot(e)], vo = sX[PN::slot(e - win)];
        const bool oi = vi == vi, oo = vo == vo;
        s = (s + (oi ? vi : 0.0)) - (oo ? vo : 0.0);
        nobs += (int)oi - (int)oo;
        neg += (int)(oi && signbit(vi)) - (int)(oo && signbit(vo));
      }
      double r;
      if (!mean && nobs == 0 && minp == 0) r = 0.0;
      else if (nobs < minp || nobs <= 0) r = qnan();
      else {
        // pandas' same-value rule: every value of the window equal to the last one
        bool same;
        double last;
        if (nobs == win) {   // no missing value: the run start decides
          last = sX[PN::slot(e)];
          same = sL[PN::slot(e)] <= tb + k - sh - win + 1;
        } else {             // missing values: compare the observed ones directly
          last = qnan();
          same = true;
          for (int j = 0; j > -win; --j) {
            const double v = sX[PN::slot(e + j)];
            if (v != v) continue;
            if (last != last) last = v;
            else same = same && v == last;
          }
        }
        if (mean) {
          r = s / (double)nobs;
          if (same) r = last;
          else if (neg == 0 && r < 0.0) r = 0.0;
          else if (neg == nobs && r > 0.0) r = 0.0;
        } else {
          r = same ? last * (double)nobs : s;
        }
      }
      res[k] = r;
    }
    store_lines<PN::K>(out, tb, T, vout, res);
    if (t0 + PN::TT >= T) break;
    __syncthreads();   // every read of this tile's ring is done
    if (pb >= PN::TT) {
#pragma unroll
      for (int k = 0; k < PN::K; ++k) {
        sX[PN::slot(pb + k - PN::TT)] = c[k];
        sL[PN::slot(pb + k - PN::TT)] = lcl[k];
      }
    }
    if (tid == PN::NT - 1) sCar = lcl[PN::K - 1];
  }
}

// ---- ewm ------------------------------------------------------------------------------
// TR: the series is the true range max(h - l, |h - c[t-1]|, |l - c[t-1]|) of
// the job's (hi, lo, x = close), formed from the loads (NaN operands skipped,
// as DataFrame.max(axis=1): the first candle's is h - l) — the ATR of
// liquidation_sweep_pump.py:206-217 without a true-range column in HBM
template <bool TR>
__global__ __launch_bounds__(PN::NT) void panel_ewm_kernel(const PanelBatch B) {
  __shared__ double sA[PN::NW], sB[PN::NW];
  __shared__ double sCarry;
  __shared__ double sX[PN::TT];   // the serial replay's tile
  const PanelJob& A = B.j[blockIdx.y];
  const int64_t row = blockIdx.x;
  if (row >= A.rows) return;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const double* __restrict__ x = A.x + row * A.ld_in;
  double* __restrict__ out = A.out + row * A.ld_out;
  const int T = B.T, minp = A.minp;
  const bool vin = vec_row(A.x, A.ld_in), vout = vec_row(A.out, A.ld_out);
  const double alpha = A.alpha, om = 1.0 - alpha, den = om + alpha;
  const bool div = den != 1.0;
  const double la = om / den, lb = alpha / den;
  if (tid == 0) sCarry = 0.0;
  bool serial = false;
  double wv = qnan(), owt = 1.0;   // pandas' state (thread 0) once the row turns serial
  int nobs = 0;
  double nx[PN::K], nh[TR ? PN::K : 1], nl[TR ? PN::K : 1];
  const double* __restrict__ xh = TR ? A.hi + row * A.ld_in : nullptr;
  const double* __restrict__ xl = TR ? A.lo + row * A.ld_in : nullptr;
  const bool vhl = TR && vec_row(A.hi, A.ld_in) && vec_row(A.lo, A.ld_in);
  auto load_tile = [&](int tb) {
    load_lane<PN::K>(x, tb, T, vin, nx);
    if constexpr (TR) {
      load_lane<PN::K>(xh, tb, T, vhl, nh);
      load_lane<PN::K>(xl, tb, T, vhl, nl);
    }
  };
  load_tile(PN::K * tid);
  for (int t0 = 0; t0 < T; t0 += PN::TT) {
    const int tb = t0 + PN::K * tid;
    double c[PN::K];
    if constexpr (TR) {
      double pc = tb >= 1 && tb <= T ? x[tb - 1] : qnan();
#pragma unroll
      for (int k = 0; k < PN::K; ++k) {
        c[k] = tb + k < T ? win_val(true_range(nh[k], nl[k], pc)) : qnan();
        pc = nx[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < PN::K; ++k) c[k] = win_val(nx[k]);   // +-inf is missing (pandas' window ops)
    }
    if (t0 + PN::TT < T) load_tile(tb + PN::TT);
    {
      int bad = 0;
#pragma unroll
      for (int k = 0; k < PN::K; ++k) bad |= (tb + k < T) && !(c[k] - c[k] == 0.0);
      if (__syncthreads_or(bad) && !serial) {
        serial = true;
        if (t0 > 0) {   // candles 0 .. t0 - 1 were all observations
          wv = sCarry;
          nobs = t0;
        }
      }
    }
    double res[PN::K];
    if (serial) {
#pragma unroll
      for (int k = 0; k < PN::K; ++k) sX[PN::K * tid + k] = c[k];
      __syncthreads();
      if (tid == 0) {
        const int n = min(PN::TT, T - t0);
        for (int i = 0; i < n; ++i) {
          const double cur = sX[i];
          const bool obs = cur == cur;
          if (t0 + i == 0) {   // pandas: weighted = vals[0], nobs = its observation
            wv = cur;
            nobs = obs ? 1 : 0;
          } else {
            nobs += obs ? 1 : 0;
            if (wv == wv) {
              owt *= om;
              if (obs) {
                if (wv != cur) {
                  wv = owt * wv + alpha * cur;
                  wv /= owt + alpha;
                }
                owt = 1.0;
              }
            } else if (obs) {
              wv = cur;
            }
          }
          sX[i] = nobs >= minp ? wv : qnan();
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PN::K; ++k) res[k] = sX[PN::K * tid + k];
      store_lines<PN::K>(out, tb, T, vout, res);
      if (t0 + PN::TT >= T) break;
      __syncthreads();
      continue;
    }
    // lane map over its candles from the zero state (candle 0 resets: a = 0, b = x)
    double a_ = 1.0, b_ = 0.0;
#pragma unroll
    for (int k = 0; k < PN::K; ++k) {
      if (tb + k == 0) {
        a_ = 0.0;
        b_ = c[k];
      } else {
        a_ *= la;
        b_ = fma(la, b_, lb * c[k]);
      }
    }
    double sa = a_, sb = b_;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const double pa = __shfl_up(sa, d, WAVE), pbv = __shfl_up(sb, d, WAVE);
      if (lane >= d) {
        sb = fma(sa, pbv, sb);
        sa *= pa;
      }
    }
    if (lane == WAVE - 1) {
      sA[w] = sa;
      sB[w] = sb;
    }
    double ea = __shfl_up(sa, 1, WAVE), eb = __shfl_up(sb, 1, WAVE);
    if (lane == 0) {
      ea = 1.0;
      eb = 0.0;
    }
    __syncthreads();
    double y = sCarry;
    for (int u = 0; u < w; ++u) y = fma(sA[u], y, sB[u]);
    y = fma(ea, y, eb);
    // exact replay of the lane's steps
#pragma unroll
    for (int k = 0; k < PN::K; ++k) {
      const int t = tb + k;
      const double v = c[k];
      if (t == 0) y = v;
      else if (y != v) {
        y = om * y + alpha * v;
        if (div) y = y / den;
      }
      res[k] = t + 1 >= minp ? y : qnan();
    }
    store_lines<PN::K>(out, tb, T, vout, res);
    if (t0 + PN::TT >= T) break;
    __syncthreads();
    if (tid == PN::NT - 1) sCarry = y;
    __syncthreads();
  }
}

bool panel_supported(int mode, int window, int shift) {
  if (mode == BQ_ROLL_EWM) return true;
  return (mode == BQ_ROLL_SUM || mode == BQ_ROLL_MEAN) && window >= 1 && shift >= 0 && window + shift <= PN::H;
}

void launch_panel(const PanelBatch& B, int n, hipStream_t st) {
  PanelBatch win, ewm;
  win.S = ewm.S = B.S;
  win.T = ewm.T = B.T;
  PanelBatch etr;
  etr.S = B.S;
  etr.T = B.T;
  int nw = 0, ne = 0, nt = 0;
  for (int i = 0; i < n; ++i) {
    if (B.j[i].mode == BQ_ROLL_EWM && B.j[i].hi) etr.j[nt++] = B.j[i];
    else if (B.j[i].mode == BQ_ROLL_EWM) ewm.j[ne++] = B.j[i];
    else win.j[nw++] = B.j[i];
  }
  if (nw) hipLaunchKernelGGL(panel_window_kernel, dim3((unsigned)B.S, (unsigned)nw), dim3(PN::NT), 0, st, win);
  if (ne) hipLaunchKernelGGL(panel_ewm_kernel<false>, dim3((unsigned)B.S, (unsigned)ne), dim3(PN::NT), 0, st, ewm);
  if (nt) hipLaunchKernelGGL(panel_ewm_kernel<true>, dim3((unsigned)B.S, (unsigned)nt), dim3(PN::NT), 0, st, etr);
}

// LiquidationSweepPump's three ewm columns in ONE pass per row
// (bq_pump_ewm): high / low / close loaded once, the true range formed from
// them, and the three series scanned side by side on the same tiles —
// panel_ewm_kernel's map scan + exact replay per series (series 1 and 2 share
// the close values; pandas' recursion on thread 0 for a series from the first
// tile with a missing / infinite value, one series at a time through sX).
// trend_score = (ema20 - ema50) / ema50 (liquidation_sweep_pump.py:254, the
// staged program's operation) leaves with them when asked, so the pump pass
// does not read the two ema columns back.
struct PumpEwmArgs {
  const double *h, *l, *c;
  double* out[3];   // atr, ema20, ema50
  double* trend;    // NULL: skip
  int64_t ld_in, ld_out;
  int T, vin, vout;
  double alpha[3];
  int minp[3];
};

// 256 threads x 8 candles (the panel kernels' 2 048-candle tile and lane maps:
// the same association as panel_ewm_kernel, so the same bits), the series one
// after another, the serial state in LDS: 111 VGPRs, 4 waves per SIMD. At
// 12.5k x 2k 0.257 ms against 0.31 / 0.30 for 512 x 4 at 4 / 8 waves per SIMD
// and 0.27 for the two panel_ewm launches it replaces (tools/ab_kernel.sh).
#ifndef BQ_P3_K
#define BQ_P3_K 8
#endif
#ifndef BQ_P3_WPS
#define BQ_P3_WPS 4
#endif
constexpr int P3_K = BQ_P3_K;
constexpr int P3_NT = 2048 / P3_K;
constexpr int P3_NW = P3_NT / WAVE;
constexpr int P3_TT = P3_NT * P3_K;

__global__ __launch_bounds__(P3_NT, BQ_P3_WPS) void pump_ewm3_kernel(const PumpEwmArgs A) {
  __shared__ double sA[P3_NW], sB[P3_NW];
  __shared__ double sCarry[3];
  __shared__ double sX[P3_TT];   // the serial replay's tile (one series at a time)
  __shared__ double sWv[3], sOwt[3];   // pandas' state of a serial series (thread 0)
  __shared__ int sNobs[3];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const double* __restrict__ xh = A.h + row * A.ld_in;
  const double* __restrict__ xl = A.l + row * A.ld_in;
  const double* __restrict__ xc = A.c + row * A.ld_in;
  const int64_t orow = row * A.ld_out;
  const int T = A.T;
  const bool vin = A.vin != 0, vout = A.vout != 0;
  if (tid < 3) {
    sCarry[tid] = 0.0;
    sWv[tid] = qnan();
    sOwt[tid] = 1.0;
    sNobs[tid] = 0;
  }
  unsigned serial = 0;   // bit e: series e runs pandas' recursion (block-uniform)
  for (int t0 = 0; t0 < T; t0 += P3_TT) {
    const int tb = t0 + P3_K * tid;
    // loaded at the tile start, not a tile ahead: registers are occupancy
    // here, and a row of up to 2 048 candles is one tile anyway
    double v[2][P3_K];   // the true range; the close (+-inf: missing)
    {
      double nh[P3_K], nl[P3_K], nc[P3_K];
      load_lane<P3_K>(xh, tb, T, vin, nh);
      load_lane<P3_K>(xl, tb, T, vin, nl);
      load_lane<P3_K>(xc, tb, T, vin, nc);
      double pc = tb >= 1 && tb <= T ? xc[tb - 1] : qnan();
#pragma unroll
      for (int k = 0; k < P3_K; ++k) {
        v[0][k] = tb + k < T ? win_val(true_range(nh[k], nl[k], pc)) : qnan();
        v[1][k] = win_val(nc[k]);
        pc = nc[k];
      }
    }
    {
      int b0 = 0, b1 = 0;
#pragma unroll
      for (int k = 0; k < P3_K; ++k) {
        b0 |= (tb + k < T) && !(v[0][k] - v[0][k] == 0.0);
        b1 |= (tb + k < T) && !(v[1][k] - v[1][k] == 0.0);
      }
      const unsigned bad = (__syncthreads_or(b0) ? 1u : 0u) | (__syncthreads_or(b1) ? 6u : 0u);
      const unsigned turn = bad & ~serial;   // these series turn serial here
      if (turn && tid == 0 && t0 > 0)        // candles 0 .. t0 - 1 were all observations
        for (int e = 0; e < 3; ++e)
          if ((turn >> e) & 1) {
            sWv[e] = sCarry[e];
            sNobs[e] = t0;
          }
      serial |= bad;
    }
    double r20[P3_K];
    // one series at a time: the lane maps over its candles from the zero
    // state (candle 0 resets), their wave scans, the waves' totals through
    // LDS, then each lane's exact replay (or pandas' recursion on thread 0)
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double al = A.alpha[e], om = 1.0 - al, den = om + al;
      const bool div = den != 1.0;
      const double* c = v[e == 0 ? 0 : 1];
      double res[P3_K];
      if ((serial >> e) & 1) {
#pragma unroll
        for (int k = 0; k < P3_K; ++k) sX[P3_K * tid + k] = c[k];
        __syncthreads();
        if (tid == 0) {
          const int n = min(P3_TT, T - t0);
          double y = sWv[e], ow = sOwt[e];
          int no = sNobs[e];
          for (int i = 0; i < n; ++i) {
            const double cur = sX[i];
            const bool obs = cur == cur;
            if (t0 + i == 0) {   // pandas: weighted = vals[0], nobs = its observation
              y = cur;
              no = obs ? 1 : 0;
            } else {
              no += obs ? 1 : 0;
              if (y == y) {
                ow *= om;
                if (obs) {
                  if (y != cur) {
                    y = ow * y + al * cur;
                    y /= ow + al;
                  }
                  ow = 1.0;
                }
              } else if (obs) {
                y = cur;
              }
            }
            sX[i] = no >= A.minp[e] ? y : qnan();
          }
          sWv[e] = y;
          sOwt[e] = ow;
          sNobs[e] = no;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < P3_K; ++k) res[k] = sX[P3_K * tid + k];
        __syncthreads();   // sX free for the next series
      } else {
        const double la = om / den, lb = al / den;
        double a_ = 1.0, b_ = 0.0;
#pragma unroll
        for (int k = 0; k < P3_K; ++k) {
          if (tb + k == 0) {
            a_ = 0.0;
            b_ = c[k];
          } else {
            a_ *= la;
            b_ = fma(la, b_, lb * c[k]);
          }
        }
        double sa = a_, sb = b_;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
          const double pa = __shfl_up(sa, d, WAVE), pbv = __shfl_up(sb, d, WAVE);
          if (lane >= d) {
            sb = fma(sa, pbv, sb);
            sa *= pa;
          }
        }
        if (lane == WAVE - 1) {
          sA[w] = sa;
          sB[w] = sb;
        }
        double ea = __shfl_up(sa, 1, WAVE), eb = __shfl_up(sb, 1, WAVE);
        if (lane == 0) {
          ea = 1.0;
          eb = 0.0;
        }
        __syncthreads();
        double y = sCarry[e];
        for (int u = 0; u < w; ++u) y = fma(sA[u], y, sB[u]);
        y = fma(ea, y, eb);
#pragma unroll
        for (int k = 0; k < P3_K; ++k) {   // exact replay of the lane's steps
          const int t = tb + k;
          const double x = c[k];
          if (t == 0) y = x;
          else if (y != x) {
            y = om * y + al * x;
            if (div) y = y / den;
          }
          res[k] = t + 1 >= A.minp[e] ? y : qnan();
        }
        __syncthreads();   // sA / sB (and sCarry[e]) read by every wave
        if (tid == P3_NT - 1) sCarry[e] = y;   // the next tile's carry (nothing reads it before then)
      }
      store_lines<P3_K>(A.out[e] + orow, tb, T, vout, res);   // each column leaves as formed
      if (e == 1) {
#pragma unroll
        for (int k = 0; k < P3_K; ++k) r20[k] = res[k];
      }
      if (e == 2 && A.trend) {
#pragma unroll
        for (int k = 0; k < P3_K; ++k) r20[k] = (r20[k] - res[k]) / res[k];
        store_lines<P3_K>(A.trend + orow, tb, T, vout, r20);
      }
    }
  }
}

}  // namespace bq

// LiquidationSweepPump's per-symbol ewm columns in panel mode
// (liquidation_sweep_pump.py:206-217, 252-254): candidate_atr =
// TR.ewm(alpha = 1/14, min_periods = 14), ema20 / ema50 of close and, when
// asked, trend_score — one pass per row (pump_ewm3_kernel).
extern "C" int bq_pump_ewm(const double* high, const double* low, const double* close, int64_t S, int64_t T,
                           int64_t ld_in, double* atr, double* ema20, double* ema50, double* trend_score,
                           int64_t ld_out, void* stream) {
  using namespace bq;
  if (!high || !low || !close || !atr || !ema20 || !ema50 || S < 0 || T < 0 || ld_in < T || ld_out < T ||
      S > 0x7fffffff || T > 0x7fffffff - 2 * P3_TT)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  PumpEwmArgs A;
  memset(&A, 0, sizeof(A));
  A.h = high;
  A.l = low;
  A.c = close;
  A.out[0] = atr;
  A.out[1] = ema20;
  A.out[2] = ema50;
  A.trend = trend_score;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  const double* const hlc[3] = {high, low, close};
  const double* const cols[4] = {atr, ema20, ema50, trend_score};
  A.vin = vec_rows(hlc, 3, ld_in);
  A.vout = vec_rows(cols, 4, ld_out);
  // pandas: alpha = 1 / (1 + com), com = 1 / alpha - 1 or (span - 1) / 2
  const double coms[3] = {1.0 / (1.0 / 14.0) - 1.0, (20.0 - 1.0) / 2.0, (50.0 - 1.0) / 2.0};
  const int minp[3] = {14, 0, 0};
  for (int i = 0; i < 3; ++i) {
    A.alpha[i] = 1.0 / (1.0 + coms[i]);
    A.minp[i] = minp[i];
  }
  hipLaunchKernelGGL(pump_ewm3_kernel, dim3((unsigned)S), dim3(P3_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
