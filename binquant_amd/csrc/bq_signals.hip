// Time-parallel kernels for the signal generators' inline helpers (SURVEY
// §8a a20) on a [S][T] panel, gfx950:
//
//   bq_wilder_rsi  MeanReversionFade._rsi          strategies/mean_reversion_fade.py:88-109
//   bq_zscore      RangeBbRsiMeanReversion._compute_zscore
//                                                  strategies/range_bb_rsi_mean_reversion.py:132-138
//   bq_adx         RangeBbRsiMeanReversion._compute_adx  (:101-130)
//
// evaluated at every candle t (column t = the helper on the prefix frame
// df.iloc[:t + 1]). The replay composition in binquant_amd.signals (exact=True)
// reproduces pandas bit for bit but is sequential per symbol (one lane per
// symbol: 12.5k symbols fill under 20 % of the SIMDs); these kernels split the
// time axis instead, at the north_star tolerance (1e-9 relative):
//
// One 256-thread workgroup per symbol walks the row in tiles of 2048 candles
// (8 consecutive candles per lane, 64-byte vector loads, the next tile
// prefetched into registers). Per-candle quantities go to an LDS ring (tile +
// 128-candle halo from the previous tile), stored lane-interleaved
// (position i at (i % 8) * (R / 8) + i / 8, so the lanes' k-th candles are
// adjacent: conflict-free). Rolling windows are one sliding walk per lane
// (w + 8 ring reads per 8 outputs). The Wilder EWMs are an associative scan of
// affine maps (wave shuffles + LDS across waves + a tile carry), after which
// each lane replays its 8 steps with pandas' exact ewm(adjust=False) update.
// pandas' rules are kept: constant windows (rolling mean returns the value,
// var returns 0), min_periods warm-up NaN, the helpers' fillna / where.
//
// Missing candles (NaN) follow pandas' rules: the z-score / ADX sliding sums
// exclude a missing value and count it (NaN while the window holds it, finite
// again once it has left); the Wilder RSI row is replayed serially with
// pandas' ewm update from the first tile holding a non-finite close (gap
// decay, observation count, a late first observation).
#include "bq_rowtile.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// 256 threads, 8 candles per lane (tiles of 2048, ring of 2176 in 8 planes of
// 272); halo 128 >= BQ_MAX_WINDOW, and twice the ADX window (bq_adx)
using SG = RowTile<256, 8, 128>;

struct SigArgs {
  const double* in[3];   // close | high, low, close
  double* out;
  int64_t ld_in, ld_out;
  int T, win;
  int vin, vout;   // 16-byte aligned rows: vector loads / stores
  double inv_w;
  double alpha, om, den;   // Wilder EWM: alpha = 1 / win, om = 1 - alpha, den = om + alpha
};

// ---- zscore ----------------------------------------------------------------------
// mean = close.rolling(w, min_periods=w).mean(), std = .std(ddof=0);
// z = 0 where std == 0 or NaN (incl. the warm-up), else (c - mean) / std.
// W > 0: the window is the reference's (20), known at compile time, so the
// window walks unroll completely (same operations, same order); W = 0: any.
template <int W>
__global__ __launch_bounds__(SG::NT) void zscore_kernel(const SigArgs A) {
  __shared__ double sC[SG::R];
  __shared__ int sW[SG::NW];
  __shared__ int sCar;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int64_t sym = blockIdx.x;
  const double* __restrict__ rc = A.in[0] + sym * A.ld_in;
  double* __restrict__ ro = A.out + sym * A.ld_out;
  const int T = A.T;
  const int win = W ? W : __builtin_amdgcn_readfirstlane(A.win);
  if (tid < SG::H) sC[SG::slot(tid)] = qnan();
  if (tid == 0) sCar = -1;
  double nx[SG::K];
  load_lane<SG::K>(rc, SG::K * tid, T, A.vin, nx);
  for (int t0 = 0; t0 < T; t0 += SG::TT) {
    const int tb = t0 + SG::K * tid, pb = SG::H + SG::K * tid;
    double c[SG::K];
#pragma unroll
    for (int k = 0; k < SG::K; ++k) c[k] = nx[k];
    if (t0 + SG::TT < T) load_lane<SG::K>(rc, tb + SG::TT, T, A.vin, nx);
#pragma unroll
    for (int k = 0; k < SG::K; ++k) sC[SG::slot(pb + k)] = c[k];
    __syncthreads();
    // last index where the close changed (pandas' same-value rule)
    int lcl[SG::K];
    {
      double pc = sC[SG::slot(pb - 1)];
      int run = -1;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        if (tb + k == 0 || c[k] != pc) run = tb + k;
        lcl[k] = run;
        pc = c[k];
      }
      const int carry = block_excl_max(lcl[SG::K - 1], &sCar, sW, lane, w);
#pragma unroll
      for (int k = 0; k < SG::K; ++k) lcl[k] = max(lcl[k], carry);
    }
    double z[SG::K];
    {
      // windows reaching before candle 0 (first tile only) hold only the
      // candles from 0 on; those outputs are warm-up, but the sliding sums
      // must not carry the halo's NaN into the first complete window
      const int gs = SG::H - t0;   // ring position of candle 0
      // a finite lane-local reference (a missing candle is excluded from the
      // sums and counted: pandas' rolling(w, min_periods=w) is NaN while the
      // window holds one, z = 0 there, and finite again once it has left)
      double r = c[0];
#pragma unroll
      for (int k = 1; k < SG::K; ++k) r = r == r ? r : c[k];
      r = r == r ? r : 0.0;
      double s1 = 0.0, s2 = 0.0;
      int nn = 0;
      auto walk = [&](int x0) {
        const double v = sC[SG::slot(pb + x0)];
        const bool ok = v == v;
        const double d = ok ? v - r : 0.0;
        nn += ok ? 0 : 1;
        s1 += d;
        s2 = fma(d, d, s2);
      };
      if (W && gs - pb <= 1 - W) {
#pragma unroll
        for (int x = 1 - W; x <= 0; ++x) walk(x);
      } else {
        for (int x = max(1 - win, gs - pb); x <= 0; ++x) walk(x);
      }
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        const int t = tb + k;
        if (k > 0) {
          const bool oi = c[k] == c[k];
          const double dn = oi ? c[k] - r : 0.0;
          const double vo = pb + k - win >= gs ? sC[SG::slot(pb + k - win)] : r;
          const bool oo = vo == vo;
          const double dol = oo ? vo - r : 0.0;
          nn += (oi ? 0 : 1) - (oo ? 0 : 1);
          s1 = (s1 + dn) - dol;
          s2 = fma(-dol, dol, fma(dn, dn, s2));
        }
        double v = 0.0;
        if (t >= win - 1 && lcl[k] > t - win + 1 && nn == 0) {
          const double var = (s2 - s1 * s1 * A.inv_w) * A.inv_w;
          const double sd = var > 0.0 ? sqrt(var) : 0.0;
          const double mean = r + s1 * A.inv_w;
          if (sd > 0.0 && sd == sd) v = (c[k] - mean) / sd;
        }
        z[k] = v;
      }
    }
    store_lines<SG::K>(ro, tb, T, A.vout, z);
    if (t0 + SG::TT >= T) break;
    __syncthreads();
    if (pb >= SG::TT) {
#pragma unroll
      for (int k = 0; k < SG::K; ++k) sC[SG::slot(pb + k - SG::TT)] = c[k];
    }
    if (tid == SG::NT - 1) sCar = lcl[SG::K - 1];
  }
}

// ---- ADX --------------------------------------------------------------------------
// tr = max(h - l, |h - pc|, |l - pc|) (skip NaN), +DM / -DM, rolling(w) sums,
// DI = 100 * sum / atr_sum, dx = 100 |DI+ - DI-| / (DI+ + DI-) (0 for a zero
// or NaN denominator, fillna(0)), adx = dx.rolling(w).mean(), 100 where NaN.
template <int W>   // as zscore_kernel (the reference's window: 14)
__global__ __launch_bounds__(SG::NT) void adx_kernel(const SigArgs A) {
  __shared__ double sTR[SG::R], sPD[SG::R], sMD[SG::R], sDX[SG::R];
  __shared__ int sW[SG::NW], sW2[SG::NW];
  __shared__ int sCar[2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int64_t sym = blockIdx.x;
  const double* __restrict__ rh = A.in[0] + sym * A.ld_in;
  const double* __restrict__ rl = A.in[1] + sym * A.ld_in;
  const double* __restrict__ rc = A.in[2] + sym * A.ld_in;
  double* __restrict__ ro = A.out + sym * A.ld_out;
  const int T = A.T;
  const int win = W ? W : __builtin_amdgcn_readfirstlane(A.win);
  if (tid < SG::H) {
    sTR[SG::slot(tid)] = sPD[SG::slot(tid)] = sMD[SG::slot(tid)] = sDX[SG::slot(tid)] = 0.0;
  }
  if (tid < 2) sCar[tid] = -1;
  double nh[SG::K], nl[SG::K], nc[SG::K];
  load_lane<SG::K>(rh, SG::K * tid, T, A.vin, nh);
  load_lane<SG::K>(rl, SG::K * tid, T, A.vin, nl);
  load_lane<SG::K>(rc, SG::K * tid, T, A.vin, nc);
  for (int t0 = 0; t0 < T; t0 += SG::TT) {
    const int tb = t0 + SG::K * tid, pb = SG::H + SG::K * tid;
    double h[SG::K], l[SG::K], c[SG::K];
#pragma unroll
    for (int k = 0; k < SG::K; ++k) {
      h[k] = nh[k];
      l[k] = nl[k];
      c[k] = nc[k];
    }
    const double ph0 = tb >= 1 && tb <= T ? rh[tb - 1] : qnan();
    const double pl0 = tb >= 1 && tb <= T ? rl[tb - 1] : qnan();
    const double pc0 = tb >= 1 && tb <= T ? rc[tb - 1] : qnan();
    if (t0 + SG::TT < T) {
      load_lane<SG::K>(rh, tb + SG::TT, T, A.vin, nh);
      load_lane<SG::K>(rl, tb + SG::TT, T, A.vin, nl);
      load_lane<SG::K>(rc, tb + SG::TT, T, A.vin, nc);
    }
    double tr[SG::K], pd[SG::K], md[SG::K];
    {
      double ph = ph0, pl = pl0, pc = pc0;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        tr[k] = true_range(h[k], l[k], pc);
        const double hd = h[k] - ph, ld = -(l[k] - pl);   // high.diff(), -low.diff()
        pd[k] = (hd > ld && hd > 0.0) ? hd : 0.0;
        md[k] = (ld > hd && ld > 0.0) ? ld : 0.0;
        sTR[SG::slot(pb + k)] = tr[k];
        sPD[SG::slot(pb + k)] = pd[k];
        sMD[SG::slot(pb + k)] = md[k];
        ph = h[k];
        pl = l[k];
        pc = c[k];
      }
    }
    __syncthreads();   // the ring (incl. the neighbour lanes' candles) is visible
    // constant-run starts of the three series (pandas' same-value rule for sums)
    int ltr[SG::K];
    {
      double ptr = sTR[SG::slot(pb - 1)], ppd = sPD[SG::slot(pb - 1)], pmd = sMD[SG::slot(pb - 1)];
      int run = -1;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        if (tb + k == 0 || tr[k] != ptr || pd[k] != ppd || md[k] != pmd) run = tb + k;
        ltr[k] = run;
        ptr = tr[k];
        ppd = pd[k];
        pmd = md[k];
      }
      const int carry = block_excl_max(ltr[SG::K - 1], &sCar[0], sW, lane, w);
#pragma unroll
      for (int k = 0; k < SG::K; ++k) ltr[k] = max(ltr[k], carry);
    }
    // dx of the lane's candles
    double dx[SG::K];
    {
      // a true range that is NaN (a missing high / low / previous close the
      // skip-NaN max cannot cover) is excluded from the sliding sum and
      // counted: pandas' rolling(w).sum() is NaN while the window holds it
      // (dx = 0) and finite again once it has left
      double st = 0.0, sp = 0.0, sm = 0.0;
      int nn = 0;
      walk_window<(W > 0)>(1 - win, [&](int x) {
        const double a = sTR[SG::slot(pb + x)];
        st += a == a ? a : 0.0;
        nn += a == a ? 0 : 1;
        sp += sPD[SG::slot(pb + x)];
        sm += sMD[SG::slot(pb + x)];
      });
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        const int t = tb + k;
        if (k > 0) {
          const int o = SG::slot(pb + k - win);
          const double ai = tr[k], ao = sTR[o];
          st = (st + (ai == ai ? ai : 0.0)) - (ao == ao ? ao : 0.0);
          nn += (ai == ai ? 0 : 1) - (ao == ao ? 0 : 1);
          sp = (sp + pd[k]) - sPD[o];
          sm = (sm + md[k]) - sMD[o];
        }
        double v = 0.0;
        if (t >= win - 1) {
          double a = nn ? qnan() : st, p = sp, m = sm;
          if (ltr[k] <= t - win + 1) {   // constant window: value * nobs
            a = tr[k] * (double)win;
            p = pd[k] * (double)win;
            m = md[k] * (double)win;
          }
          const double pdi = 100.0 * p / a, mdi = 100.0 * m / a;
          const double tot = pdi + mdi;
          v = tot != 0.0 ? 100.0 * fabs(pdi - mdi) / tot : qnan();
          if (v != v) v = 0.0;
        }
        dx[k] = v;
        sDX[SG::slot(pb + k)] = v;
      }
    }
    __syncthreads();   // dx of every lane visible
    int ldx[SG::K];
    {
      double pv = sDX[SG::slot(pb - 1)];
      int run = -1;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        if (tb + k == 0 || dx[k] != pv) run = tb + k;
        ldx[k] = run;
        pv = dx[k];
      }
      const int carry = block_excl_max(ldx[SG::K - 1], &sCar[1], sW2, lane, w);
#pragma unroll
      for (int k = 0; k < SG::K; ++k) ldx[k] = max(ldx[k], carry);
    }
    double adx[SG::K];
    {
      double s = 0.0;
      walk_window<(W > 0)>(1 - win, [&](int x) { s += sDX[SG::slot(pb + x)]; });
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        const int t = tb + k;
        if (k > 0) s = (s + dx[k]) - sDX[SG::slot(pb + k - win)];
        double v = 100.0;
        if (t >= win - 1) {
          if (ldx[k] <= t - win + 1) v = dx[k];
          else v = div_exact(s < 0.0 ? 0.0 : s, (double)win, A.inv_w);
        }
        adx[k] = v;
      }
    }
    store_lines<SG::K>(ro, tb, T, A.vout, adx);
    if (t0 + SG::TT >= T) break;
    __syncthreads();
    if (pb >= SG::TT) {
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        const int d = SG::slot(pb + k - SG::TT);
        sTR[d] = tr[k];
        sPD[d] = pd[k];
        sMD[d] = md[k];
        sDX[d] = dx[k];
      }
    }
    if (tid == SG::NT - 1) {
      sCar[0] = ltr[SG::K - 1];
      sCar[1] = ldx[SG::K - 1];
    }
  }
}

// ---- Wilder RSI ----------------------------------------------------------------
// gain / loss = delta.clip(lower=0) / -delta.clip(upper=0) (NaN at candle 0),
// avg = ewm(alpha = 1 / w, min_periods = w, adjust=False).mean() (the first
// observation, candle 1, starts the average), rsi = 100 avg_g / (avg_g +
// avg_l), 50 where the denominator is 0, NaN during the warm-up.
template <bool DIV>
__device__ __forceinline__ double wilder_step(double y, double x, const SigArgs& A) {
  if (y != x) {
    y = A.om * y + A.alpha * x;
    if (DIV) y = y / A.den;
  }
  return y;
}

template <bool DIV>
__global__ __launch_bounds__(SG::NT) void wilder_rsi_kernel(const SigArgs A) {
  __shared__ double sA[SG::NW], sB[2][SG::NW];
  __shared__ double sCarry[2];
  __shared__ double sX[SG::TT];   // the serial replay's tile (rows with missing candles)
  __shared__ double sSt[4];      // its pandas state: avg gain, avg loss, old weight, previous close
  __shared__ int sNobs;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int64_t sym = blockIdx.x;
  const double* __restrict__ rc = A.in[0] + sym * A.ld_in;
  double* __restrict__ ro = A.out + sym * A.ld_out;
  const int T = A.T;
  // the scan's per-candle map: y -> la * y + lb * x (la = om / den, lb = alpha / den)
  const double la = A.om / A.den, lb = A.alpha / A.den;
  if (tid < 2) sCarry[tid] = 0.0;
  // pandas' ewm state once the row turns serial (LDS, thread 0): averages,
  // old weight, previous close, observation count
  bool serial = false;
  if (tid == 0) {
    sSt[0] = sSt[1] = sSt[3] = qnan();
    sSt[2] = 1.0;
    sNobs = 0;
  }
  double nx[SG::K];
  load_lane<SG::K>(rc, SG::K * tid, T, A.vin, nx);
  for (int t0 = 0; t0 < T; t0 += SG::TT) {
    const int tb = t0 + SG::K * tid;
    double c[SG::K];
#pragma unroll
    for (int k = 0; k < SG::K; ++k) c[k] = nx[k];
    const double pc0 = tb >= 1 && tb <= T ? rc[tb - 1] : qnan();
    if (t0 + SG::TT < T) load_lane<SG::K>(rc, tb + SG::TT, T, A.vin, nx);
    // A missing (NaN) or infinite close breaks the scan's fixed per-candle
    // map: pandas' ewm(ignore_na=False) decays the old weight across a gap
    // and divides by (old_wt + alpha), counts only observations toward
    // min_periods and starts at the first observation wherever it is. From
    // the first tile holding one, the row is replayed serially with pandas'
    // own update (thread 0; the carry so far seeds it) — exact, and only the
    // rows with gaps pay for it.
    {
      int bad = 0;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) bad |= (tb + k < T) && !(c[k] - c[k] == 0.0);
      if (__syncthreads_or(bad) && !serial) {
        serial = true;
        if (t0 > 0 && tid == 0) {   // candles 1 .. t0 - 1 were all observations
          sSt[0] = sCarry[0];
          sSt[1] = sCarry[1];
          sSt[3] = rc[t0 - 1];
          sNobs = t0 - 1;
        }
      }
    }
    if (serial) {
#pragma unroll
      for (int k = 0; k < SG::K; ++k) sX[SG::K * tid + k] = c[k];
      __syncthreads();
      if (tid == 0) {
        double wg = sSt[0], wl = sSt[1], owt = sSt[2], prev = sSt[3];
        int nobs = sNobs;
        const int n = min(SG::TT, T - t0);
        for (int i = 0; i < n; ++i) {
          const double cur = sX[i];
          const double d = cur - prev;
          prev = cur;
          const double g = d != d ? d : (d > 0.0 ? d : 0.0);
          const double l = d != d ? d : (d < 0.0 ? -d : 0.0);
          const bool obs = g == g;
          nobs += obs ? 1 : 0;
          if (wg == wg) {
            owt *= A.om;
            if (obs) {
              if (wg != g) {
                wg = owt * wg + A.alpha * g;
                wg /= owt + A.alpha;
              }
              if (wl != l) {
                wl = owt * wl + A.alpha * l;
                wl /= owt + A.alpha;
              }
              owt = 1.0;
            }
          } else if (obs) {
            wg = g;
            wl = l;
          }
          double v = qnan();
          if (nobs >= A.win) {
            const double den = wg + wl;
            v = den != 0.0 ? (100.0 * wg) / den : 50.0;
          }
          sX[i] = v;
        }
        sSt[0] = wg;
        sSt[1] = wl;
        sSt[2] = owt;
        sSt[3] = prev;
        sNobs = nobs;
      }
      __syncthreads();
      double rsi[SG::K];
#pragma unroll
      for (int k = 0; k < SG::K; ++k) rsi[k] = sX[SG::K * tid + k];
      store_lines<SG::K>(ro, tb, T, A.vout, rsi);
      if (t0 + SG::TT >= T) break;
      __syncthreads();
      continue;
    }
    double g[SG::K], l[SG::K];
    {
      double pc = pc0;
#pragma unroll
      for (int k = 0; k < SG::K; ++k) {
        const double d = c[k] - pc;
        g[k] = d != d ? d : (d > 0.0 ? d : 0.0);
        l[k] = d != d ? d : (d < 0.0 ? -d : 0.0);
        pc = c[k];
      }
    }
    // lane map over its K candles from the zero state; candle 1 (the first
    // observation) resets the state: a = 0, b = x
    double A_ = 1.0, Bg = 0.0, Bl = 0.0;
#pragma unroll
    for (int k = 0; k < SG::K; ++k) {
      const int t = tb + k;
      if (t == 0) continue;   // NaN observation before any: no state
      if (t == 1) {
        A_ = 0.0;
        Bg = g[k];
        Bl = l[k];
      } else {
        A_ *= la;
        Bg = fma(la, Bg, lb * g[k]);
        Bl = fma(la, Bl, lb * l[k]);
      }
    }
    // block exclusive scan of (A, Bg, Bl): wave Hillis-Steele with shuffles
    double sa = A_, sg = Bg, sl = Bl;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const double pa = __shfl_up(sa, d, WAVE), pg = __shfl_up(sg, d, WAVE), pl = __shfl_up(sl, d, WAVE);
      if (lane >= d) {   // (sa, sg) after (pa, pg)
        sg = fma(sa, pg, sg);
        sl = fma(sa, pl, sl);
        sa *= pa;
      }
    }
    if (lane == WAVE - 1) {
      sA[w] = sa;
      sB[0][w] = sg;
      sB[1][w] = sl;
    }
    // exclusive within the wave
    double ea = __shfl_up(sa, 1, WAVE), eg = __shfl_up(sg, 1, WAVE), el = __shfl_up(sl, 1, WAVE);
    if (lane == 0) {
      ea = 1.0;
      eg = el = 0.0;
    }
    __syncthreads();
    double yg = sCarry[0], yl = sCarry[1];
    for (int u = 0; u < w; ++u) {
      yg = fma(sA[u], yg, sB[0][u]);
      yl = fma(sA[u], yl, sB[1][u]);
    }
    yg = fma(ea, yg, eg);
    yl = fma(ea, yl, el);
    // exact replay of the lane's K steps
    double rsi[SG::K];
#pragma unroll
    for (int k = 0; k < SG::K; ++k) {
      const int t = tb + k;
      if (t == 1) {
        yg = g[k];
        yl = l[k];
      } else if (t > 1) {
        yg = wilder_step<DIV>(yg, g[k], A);
        yl = wilder_step<DIV>(yl, l[k], A);
      }
      double v = qnan();
      if (t >= A.win && t < T) {   // nobs (candles 1..t) >= min_periods
        const double den = yg + yl;
        v = den != 0.0 ? (100.0 * yg) / den : 50.0;
      }
      rsi[k] = v;
    }
    store_lines<SG::K>(ro, tb, T, A.vout, rsi);
    if (t0 + SG::TT >= T) break;
    __syncthreads();
    if (tid == SG::NT - 1) {
      sCarry[0] = yg;
      sCarry[1] = yl;
    }
    __syncthreads();
  }
}

// 16-byte vector access needs every row start 16-byte aligned
static void set_vec(SigArgs& A, int64_t ld_in, int64_t ld_out, int n_in) {
  A.vin = vec_rows(A.in, n_in, ld_in);
  A.vout = vec_rows(&A.out, 1, ld_out);
}

static bool sig_ok(const void* a, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, const void* out, int w,
                   int wmax) {
  return a && out && S >= 0 && T >= 0 && ld_in >= T && ld_out >= T && T <= 0x7fffffff - 2 * SG::TT &&
         S <= 0x7fffffff && w >= 1 && w <= wmax;
}

}  // namespace bq

extern "C" {

int bq_zscore(const double* close, int64_t S, int64_t T, int64_t ld_in, int32_t window, double* out, int64_t ld_out,
              void* stream) {
  using namespace bq;
  if (!sig_ok(close, S, T, ld_in, ld_out, out, window, BQ_MAX_WINDOW)) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  SigArgs A;
  memset(&A, 0, sizeof A);
  A.in[0] = close;
  A.out = out;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.win = window;
  A.inv_w = 1.0 / (double)window;
  set_vec(A, ld_in, ld_out, 1);
  if (window == 20) hipLaunchKernelGGL(zscore_kernel<20>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(zscore_kernel<0>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

int bq_adx(const double* high, const double* low, const double* close, int64_t S, int64_t T, int64_t ld_in,
           int32_t window, double* out, int64_t ld_out, void* stream) {
  using namespace bq;
  // the mean of dx reaches 2 (w - 1) candles back: inside the 128-candle halo
  if (!high || !low || !sig_ok(close, S, T, ld_in, ld_out, out, window, SG::H / 2)) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  SigArgs A;
  memset(&A, 0, sizeof A);
  A.in[0] = high;
  A.in[1] = low;
  A.in[2] = close;
  A.out = out;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.win = window;
  A.inv_w = 1.0 / (double)window;
  set_vec(A, ld_in, ld_out, 3);
  if (window == 14) hipLaunchKernelGGL(adx_kernel<14>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(adx_kernel<0>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

int bq_wilder_rsi(const double* close, int64_t S, int64_t T, int64_t ld_in, int32_t window, double* out,
                  int64_t ld_out, void* stream) {
  using namespace bq;
  if (!sig_ok(close, S, T, ld_in, ld_out, out, window, 1 << 20)) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  SigArgs A;
  memset(&A, 0, sizeof A);
  A.in[0] = close;
  A.out = out;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.win = window;
  // pandas: ewm(alpha = 1 / w) keeps com = 1 / alpha - 1 and recomputes
  // alpha = 1 / (1 + com); old_wt_factor = 1 - alpha, new_wt = alpha
  A.alpha = 1.0 / (1.0 + (1.0 / (1.0 / (double)window) - 1.0));
  A.om = 1.0 - A.alpha;
  A.den = A.om + A.alpha;
  set_vec(A, ld_in, ld_out, 1);
  if (A.den != 1.0)
    hipLaunchKernelGGL(wilder_rsi_kernel<true>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(wilder_rsi_kernel<false>, dim3((unsigned)S), dim3(SG::NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // extern "C"
