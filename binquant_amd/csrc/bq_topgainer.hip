// TopGainerEarlyMomentum on a [S][T] panel (gfx950): the features of every
// prefix frame (_features, strategies/top_gainer_early_momentum.py:91-159),
// the 11-step breakout gate (_entry_allows, :161-188), signal()'s two-close
// confirmation and risk branch (:190-202, :363-406) and the candidate candle's
// score / stop loss (:236-253) in ONE pass over the row. Column t of row s =
// the reference run on the frame df.iloc[first:t + 1], first = first_t[s].
//
// Mapping (bq_rowtile.h): one 256-thread workgroup per symbol walks its row in
// tiles of 1024 candles, 4 per lane; an LDS ring with a 96-candle halo holds
// high, close, volume and the quote volume (candles before `first` as NaN), so
// the 48-high window, the 32-candle volume windows, close[t - 4 / 8 / 24] and
// the t - 96 extension anchor read the ring and every input byte crosses HBM
// once. Per tile:
//   A. the lane's candles go to the ring; the two ewm series (close, span 20
//      and 50, seeded at `first`) as in bq_pump_features_ewm: the lanes' affine
//      maps y -> a y + b x over their 4 candles (zero before `first`, so the
//      seed's lane receives a zero carry), a DPP wave scan, the waves' totals
//      through LDS, the tile carry, then each lane replays its 4 steps with
//      pandas' update. A row that meets a missing or infinite close inside its
//      frame continues serially from that tile with pandas' own recursion
//      (thread 0, from the ring, results through an LDS line).
//   C. per candle: the windows (a lane's 4 windows share all but 3 elements:
//      the common part is walked once), the 21 values in the reference's
//      operation order, the feature status, the gate as a priority encode of
//      selects, and the breakout candle's score. The candle two back — its
//      gate, previous_high and score — is the lane's own k - 2 or the
//      neighbouring lane's (DPP wave_shr:1; a wave's first lane reads the
//      previous wave's, or the previous tile's, through LDS): carried, not
//      recomputed.
// Nothing is written but the requested outputs: 40-56 B in, up to 186 B out
// per candle. The point-wise values are one or two correctly rounded fp64
// operations each (bit-exact); the window means are fresh sums of the window
// (no sliding cancellation: the sign clamps of pandas' roll_mean cannot fire)
// with its same-value rule (min == max over a full window), within rounding
// of pandas' compensated sum. Rounding score / stop_loss_pct (pybinbot's
// round_numbers) is the host's step.
#include "bq_rowtile.h"
#include "binquant_amd.h"

#include <stdint.h>
#include <string.h>

namespace bq {

using TG = RowTile<256, 4, BQ_TGE_MAX_LOOKBACK>;

// one ewm series: pandas' alpha / old-weight factor / divisor, the affine map
// y -> la y + lb x, apow[j] = la^(4 * 2^j), mw = la^(4 * 64) (one wave's span)
struct TgEwm {
  double alpha, om, den, la, lb, mw;
  double apow[8];
  int div;
};

struct TgArgs {
  const double *open, *high, *low, *close, *volume, *qv, *atr;
  const uint8_t* risk;
  const int64_t *lens, *first;
  int64_t ld_in, ld_qv, ld_atr, ld_risk, ld_out;
  int T;
  bq_top_gainer_params p;
  TgEwm ew[2];   // span 20, span 50
  uint8_t *status, *entry;
  double *score, *stop;
  double* val[BQ_TGE_NVALUES];
};

enum { TG_VIN = 1, TG_VQV = 2, TG_VATR = 4, TG_VOUT = 8, TG_VBYTES = 16 };

// py_min / py_max (bq_device.h): the second argument wins only when the
// comparison holds, so a NaN first argument sticks and a NaN second is skipped

struct TgMax {   // Series.max(): NaN-skipping, NaN when nothing is left
  double m = qnan();
  __device__ __forceinline__ void add(double v) { m = fmax(m, v); }
};

struct TgMean {   // rolling(W).mean(): observations, their sum, min and max
  double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  int n = 0;
  __device__ __forceinline__ void add(double v) {
    const bool ok = win_ok(v);   // NaN and +-inf are missing (window op)
    s += ok ? v : 0.0;
    n += ok;
    mn = fmin(mn, v);
    mx = fmax(mx, v);
  }
  // min_periods = window; every value equal: that value (the same-value rule)
  __device__ __forceinline__ double mean(int W) const { return n < W ? qnan() : (mn == mx ? mn : s / (double)n); }
};

// The windows [base + k - W + 1, base + k] of a lane's candles k = 0 .. 3 in
// ring positions: the part common to the four walked once, the up to three
// elements on either side per candle. WC > 0: W as a compile-time constant
// (the walks unroll, the ring slots become immediate offsets).
template <int WC, typename Acc, typename Rd>
__device__ __forceinline__ void tg_windows(int base, int Wrt, Rd&& rd, Acc (&acc)[TG::K]) {
  const int W = WC > 0 ? WC : Wrt;
  Acc common;
#pragma unroll
  for (int d = TG::K - W; d <= 0; ++d) common.add(rd(base + d));   // empty for W < 4
#pragma unroll
  for (int k = 0; k < TG::K; ++k) {
    Acc a = common;
    const int hi1 = min(k, TG::K - 1 - W);
#pragma unroll
    for (int d = k - W + 1; d <= hi1; ++d) a.add(rd(base + d));
#pragma unroll
    for (int d = max(1, hi1 + 1); d <= k; ++d) a.add(rd(base + d));
    acc[k] = a;
  }
}

// a lane's 4 codes of consecutive candles: one 4-byte store where the row allows
__device__ __forceinline__ void put_codes(uint8_t* __restrict__ row, int tb, int T, bool vec4, const int (&b)[TG::K]) {
  if (vec4 && tb + TG::K <= T) {
    const uint32_t w = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    *reinterpret_cast<uint32_t*>(row + tb) = w;
  } else {
#pragma unroll
    for (int k = 0; k < TG::K; ++k)
      if (tb + k < T) row[tb + k] = (uint8_t)b[k];
  }
}

// 2 workgroups per CU: the 21 value columns of a lane's 4 candles are live
// until the feature status is known (DESIGN §4.19 has the register figures)
template <bool QV, int LHC = 0, int VWC = 0>
__global__ __launch_bounds__(TG::NT, 2) void top_gainer_kernel(const TgArgs A, int vflags) {
  __shared__ double sH[TG::R], sC[TG::R], sV[TG::R], sQ[QV ? TG::R : 1];
  __shared__ double sS[2][TG::TT];              // the serial path's ewm values of the tile
  __shared__ double sEB[2][TG::NW], sEC[2];     // the waves' scan totals; the ewm values at the previous tile's end
  // previous_high and score of each wave's last two candles ([0]: the
  // previous tile's), and their gate codes
  __shared__ double sTP[TG::NW + 1][2], sTS[TG::NW + 1][2];
  __shared__ int sTE[TG::NW + 1][2];
  __shared__ int sBad;   // a missing / infinite close inside the frame in this tile
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int64_t s = blockIdx.x;
  const int T = A.T;
  const bq_top_gainer_params P = A.p;
  const int LH = LHC > 0 ? LHC : P.lookback_high, VW = VWC > 0 ? VWC : P.volume_window;
  const int FE = P.full_extension_bars;
  const int64_t len64 = A.lens ? A.lens[s] : (int64_t)T;
  const int len = len64 < 0 ? 0 : len64 > T ? T : (int)len64;
  const int64_t f64 = A.first ? A.first[s] : 0;
  const int first = f64 < 0 ? 0 : f64 > T ? T : (int)f64;
  const int64_t irow = s * A.ld_in, orow = s * A.ld_out;
  const bool vin = vflags & TG_VIN, vqv = vflags & TG_VQV, vatr = vflags & TG_VATR, vout = vflags & TG_VOUT,
             vbytes = vflags & TG_VBYTES;
  if (tid < TG::H) {   // before the row: missing values
    sH[TG::slot(tid)] = sC[TG::slot(tid)] = sV[TG::slot(tid)] = qnan();
    if (QV) sQ[TG::slot(tid)] = qnan();
  }
  if (tid == 0) {
    sBad = 0;
    sEC[0] = sEC[1] = 0.0;
    sTE[0][0] = sTE[0][1] = BQ_TGE_SHORT_HISTORY;
    sTP[0][0] = sTP[0][1] = sTS[0][0] = sTS[0][1] = qnan();
  }
  // the frame's first close: the extension anchor while the frame is short
  const double c_first = first < T ? A.close[irow + first] : qnan();
  double lpow[2], rpow[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    lpow[e] = pow_bits<6>(A.ew[e].apow, lane);
    rpow[e] = pow_bits<5>(A.ew[e].apow, (lane & 15) + 1);
  }
  // the serial state (thread 0) once the row has met a missing close
  bool serial = false;
  double swv[2] = {qnan(), qnan()}, sowt[2] = {1.0, 1.0};
  __syncthreads();

  for (int t0 = 0; t0 < T; t0 += TG::TT) {
    const int tb = t0 + TG::K * tid, pb = TG::H + TG::K * tid;
    double o[TG::K], h[TG::K], l[TG::K], c[TG::K], v[TG::K], q[TG::K], atr[TG::K];
    int rk[TG::K];
    load_lane<TG::K>(A.open + irow, tb, T, vin, o);
    load_lane<TG::K>(A.high + irow, tb, T, vin, h);
    load_lane<TG::K>(A.low + irow, tb, T, vin, l);
    load_lane<TG::K>(A.close + irow, tb, T, vin, c);
    load_lane<TG::K>(A.volume + irow, tb, T, vin, v);
    if (QV) load_lane<TG::K>(A.qv + s * A.ld_qv, tb, T, vqv, q);
    if (A.atr) load_lane<TG::K>(A.atr + s * A.ld_atr, tb, T, vatr, atr);
#pragma unroll
    for (int k = 0; k < TG::K; ++k) {
      const int t = tb + k;
      if (!A.atr) atr[k] = 0.0;   // no ATR column (:120)
      rk[k] = A.risk && t < T ? A.risk[s * A.ld_risk + t] : 1;
      if (t < first) o[k] = h[k] = l[k] = c[k] = v[k] = q[k] = qnan();   // not in the frame
      if (!QV) q[k] = v[k] * c[k];                                       // :113
    }
    // ---- phase A: the ring, the ewm series' lane maps and wave scans
    double sv[TG::K], ewx[2], e20[TG::K], e50[TG::K], ewy[2] = {0.0, 0.0};
    {
      int bad = 0;
#pragma unroll
      for (int k = 0; k < TG::K; ++k) {
        const int t = tb + k;
        sH[TG::slot(pb + k)] = h[k];
        sC[TG::slot(pb + k)] = c[k];
        sV[TG::slot(pb + k)] = v[k];
        if (QV) sQ[TG::slot(pb + k)] = q[k];
        sv[k] = t < first ? 0.0 : win_val(c[k]);   // ewm: +-inf is missing
        bad |= t >= first && t < len && !(sv[k] == sv[k]);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < TG::K; ++k) y = tb + k == first ? sv[k] : fma(A.ew[e].la, y, A.ew[e].lb * sv[k]);
        const double inc = wave_scan_affine_dpp_rp(y, A.ew[e].apow, rpow[e], lane);
        if (lane == WAVE - 1) sEB[e][w] = inc;
        ewx[e] = dpp_f64<DPP_WAVE_SHR1>(inc);   // exclusive (lane 0: the carry alone)
      }
      if (bad) atomicOr(&sBad, 1);
    }
    __syncthreads();   // A: ring, wave totals, sBad
    if (sBad && !serial) {   // block-uniform (from LDS): the row turns serial here
      serial = true;
      if (t0 > first) {   // candles first .. t0 - 1 were all observations
        swv[0] = sEC[0];
        swv[1] = sEC[1];
      }
    }
    if (serial) {
      if (tid == 0) {   // pandas' recursion over the tile, both series
        const int n = min(TG::TT, T - t0);
        for (int i = 0; i < n; ++i) {
          const int t = t0 + i;
          const double cur = win_val(sC[TG::slot(TG::H + i)]);
          const bool obs = cur == cur;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            double wv = swv[e], owt = sowt[e];
            if (t == first) {
              wv = cur;
              owt = 1.0;
            } else if (t > first) {
              if (wv == wv) {
                owt *= A.ew[e].om;
                if (obs) {
                  if (wv != cur) {
                    wv = owt * wv + A.ew[e].alpha * cur;
                    wv /= owt + A.ew[e].alpha;
                  }
                  owt = 1.0;
                }
              } else if (obs) {
                wv = cur;
              }
            }
            swv[e] = wv;
            sowt[e] = owt;
            sS[e][(i & (TG::K - 1)) * TG::NT + i / TG::K] = wv;   // lane-interleaved, as the ring
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < TG::K; ++k) {
        e20[k] = sS[0][k * TG::NT + tid];
        e50[k] = sS[1][k * TG::NT + tid];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const TgEwm& E = A.ew[e];
        // the value at candle tb - 1: the carry through the earlier waves'
        // totals, then this lane's exclusive prefix
        double y = sEC[e];
        for (int u = 0; u < w; ++u) y = fma(E.mw, y, sEB[e][u]);
        y = lane == 0 ? y : fma(lpow[e], y, ewx[e]);
#pragma unroll
        for (int k = 0; k < TG::K; ++k) {   // pandas' update, step by step
          const double x = sv[k];
          if (tb + k == first) y = x;
          else if (y != x) {
            y = E.om * y + E.alpha * x;
            if (E.div) y = y / E.den;
          }
          (e == 0 ? e20 : e50)[k] = y;
        }
        ewy[e] = y;
      }
    }

    // ---- phase C: the lane's 4 candles
    const bool whole = t0 + TG::TT <= T;
    double ph[TG::K], vma[TG::K], qvma[TG::K];
    {   // one window family at a time: its accumulators die before the next
      TgMean acc[TG::K];
      tg_windows<VWC>(pb, VW, [&](int p) { return sV[TG::slot(p)]; }, acc);   // :109
#pragma unroll
      for (int k = 0; k < TG::K; ++k) vma[k] = acc[k].mean(VW);
    }
    if (QV) {
      TgMean acc[TG::K];
      tg_windows<VWC>(pb, VW, [&](int p) { return sQ[TG::slot(p)]; }, acc);   // :116
#pragma unroll
      for (int k = 0; k < TG::K; ++k) qvma[k] = acc[k].mean(VW);
    } else {
#pragma unroll
      for (int k = 0; k < TG::K; ++k) qvma[k] = vma[k] * c[k];   // :118
    }
    {
      TgMax acc[TG::K];
      tg_windows<LHC>(pb - 1, LH, [&](int p) { return sH[TG::slot(p)]; }, acc);   // the LH highs before t (:108)
#pragma unroll
      for (int k = 0; k < TG::K; ++k) ph[k] = acc[k].m;
    }
    double r1[TG::K], r2[TG::K], r6[TG::K], ext[TG::K], bars[TG::K], cap[TG::K], cr[TG::K], vr[TG::K],
        qvr[TG::K], rp[TG::K], uwf[TG::K], sc[TG::K];
    int en[TG::K];
    bool rdy[TG::K];
#pragma unroll
    for (int k = 0; k < TG::K; ++k) {
      const int t = tb + k, p = pb + k;
      const int n = t + 1 - first;   // len(df)
      const double rng = h[k] - l[k];                          // :122
      const double uw = h[k] - py_max(o[k], c[k]);             // :123
      // :124-132
      const int nb = min(n - 1, FE);
      const double anchor = t - first >= FE ? sC[TG::slot(p - FE)] : c_first;
      bars[k] = (double)nb;
      cap[k] = nb < FE ? py_max(P.min_short_extension_cap, P.max_extension * (bars[k] / (double)FE)) : P.max_extension;
      r1[k] = c[k] / sC[TG::slot(p - 4)] - 1.0;
      r2[k] = c[k] / sC[TG::slot(p - 8)] - 1.0;
      r6[k] = c[k] / sC[TG::slot(p - 24)] - 1.0;
      ext[k] = c[k] / anchor - 1.0;
      cr[k] = c[k] / o[k] - 1.0;
      vr[k] = v[k] / (vma[k] + 1e-6);
      qvr[k] = q[k] / (qvma[k] + 1e-6);
      rp[k] = (c[k] - l[k]) / (rng + 1e-6);
      uwf[k] = uw / (rng + 1e-6);
      // the feature status, in the method's order (:93, :105, :157)
      const bool f_short = n < P.min_history;
      double m = c[k];   // Python's min(close, open, high, low, volume)
      m = py_min(m, o[k]);
      m = py_min(m, h[k]);
      m = py_min(m, l[k]);
      m = py_min(m, v[k]);
      const bool f_inv = m <= 0.0;
      const bool fin = is_finite(c[k]) && is_finite(o[k]) && is_finite(h[k]) && is_finite(l[k]) && is_finite(v[k]) &&
                       is_finite(q[k]) && is_finite(ph[k]) && is_finite(r1[k]) && is_finite(r2[k]) &&
                       is_finite(r6[k]) && is_finite(ext[k]) && is_finite(cap[k]) && is_finite(cr[k]) &&
                       is_finite(vr[k]) && is_finite(qvr[k]) && is_finite(rp[k]) && is_finite(uwf[k]) &&
                       is_finite(e20[k]) && is_finite(e50[k]) && is_finite(atr[k]);
      // _entry_allows (:163-187): the first failing check, selects from the last to the first
      int st = BQ_TGE_CONFIRMED;
      st = uwf[k] > P.max_upper_wick ? BQ_TGE_UPPER_WICK : st;
      st = rp[k] < P.min_range_position ? BQ_TGE_NOT_NEAR_HIGH : st;
      st = vr[k] < P.min_volume_ratio ? BQ_TGE_VOLUME_LOW : st;
      st = r6[k] < P.min_return_6h ? BQ_TGE_SIX_HOUR : st;
      st = ((r1[k] < P.min_return_1h) & (r2[k] < P.min_return_2h)) ? BQ_TGE_NOT_ACCELERATING : st;
      st = ext[k] > cap[k] ? BQ_TGE_EXTENSION : st;
      st = r1[k] > P.max_return_1h ? BQ_TGE_HOUR_EXTENDED : st;
      st = cr[k] > P.max_candle_return ? BQ_TGE_CANDLE_EXTENDED : st;
      st = cr[k] < P.min_candle_return ? BQ_TGE_NOT_GREEN : st;
      st = ((c[k] <= e20[k]) | (c[k] <= e50[k])) ? BQ_TGE_NOT_ABOVE_EMAS : st;
      st = c[k] <= ph[k] ? BQ_TGE_NOT_BREAKING : st;
      st = !fin ? BQ_TGE_NOT_READY : st;
      st = f_inv ? BQ_TGE_INVALID_CANDLE : st;
      st = f_short ? BQ_TGE_SHORT_HISTORY : st;
      st = t >= len ? BQ_TGE_NO_FRAME : st;
      en[k] = st;
      rdy[k] = !f_short && !f_inv && fin && t < len;
      // _score (:246-253), unrounded
      sc[k] = ((1.0 + py_min(r1[k] * 4.0, 0.8)) + py_min(vr[k] / 10.0, 0.5)) + py_min(rp[k] / 4.0, 0.25);
    }
    put_codes(A.entry + orow, tb, T, vbytes, en);
    auto put = [&](int col, const double (&x)[TG::K]) {
      if (!A.val[col]) return;   // wave-uniform: a NULL column is skipped
      double r[TG::K];
#pragma unroll
      for (int k = 0; k < TG::K; ++k) r[k] = rdy[k] ? x[k] : qnan();
      store_lines<TG::K>(A.val[col] + orow, tb, T, vout, r, whole);
    };
    put(0, c);
    put(1, o);
    put(2, h);
    put(3, l);
    put(4, v);
    put(5, q);
    put(6, ph);
    put(7, r1);
    put(8, r2);
    put(9, r6);
    put(10, ext);
    put(11, bars);
    put(12, cap);
    put(13, cr);
    put(14, vr);
    put(15, qvr);
    put(16, rp);
    put(17, uwf);
    put(18, e20);
    put(19, e50);
    put(20, atr);

    // ---- the breakout candle t - 2: the lane's own k - 2, or the lane before
    int pe[2] = {dpp_i32<DPP_WAVE_SHR1>(en[2]), dpp_i32<DPP_WAVE_SHR1>(en[3])};
    double pp[2] = {dpp_f64<DPP_WAVE_SHR1>(ph[2]), dpp_f64<DPP_WAVE_SHR1>(ph[3])};
    double ps[2] = {dpp_f64<DPP_WAVE_SHR1>(sc[2]), dpp_f64<DPP_WAVE_SHR1>(sc[3])};
    if (lane == WAVE - 1) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sTE[w + 1][j] = en[2 + j];
        sTP[w + 1][j] = ph[2 + j];
        sTS[w + 1][j] = sc[2 + j];
      }
    }
    __syncthreads();   // the waves' last candles
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        pe[j] = sTE[w][j];
        pp[j] = sTP[w][j];
        ps[j] = sTS[w][j];
      }
    }
    int stt[TG::K];
    double score[TG::K], stop[TG::K];
#pragma unroll
    for (int k = 0; k < TG::K; ++k) {
      const int t = tb + k, p = pb + k;
      const int e2 = k < 2 ? pe[k] : en[k - 2];
      const double ph2 = k < 2 ? pp[k] : ph[k - 2], sc2 = k < 2 ? ps[k] : sc[k - 2];
      const double c1 = sC[TG::slot(p - 1)], c2 = sC[TG::slot(p - 2)];
      // signal() (:363-406), selects from the last check to the first
      int st = BQ_TGE_CONFIRMED;
      st = rk[k] == 0 ? BQ_TGE_RISK_REJECTED : st;
      st = c[k] <= c2 ? BQ_TGE_SECOND_CONFIRM : st;
      st = c1 <= ph2 ? BQ_TGE_FIRST_CONFIRM : st;
      st = e2 != BQ_TGE_CONFIRMED ? e2 : st;
      st = t + 1 - first < P.min_history + 2 ? BQ_TGE_SHORT_HISTORY : st;
      st = t >= len ? BQ_TGE_NO_FRAME : st;
      stt[k] = st;
      const bool cand = st == BQ_TGE_CONFIRMED || st == BQ_TGE_RISK_REJECTED;
      // _stop_loss_pct (:236-243), unrounded
      const double pct = ((P.atr_stop_mult * atr[k]) / c[k]) * 100.0;
      const double sl = ((c[k] <= 0.0) | (atr[k] <= 0.0))
                            ? P.min_stop_loss_pct
                            : py_min(py_max(pct, P.min_stop_loss_pct), P.max_stop_loss_pct);
      score[k] = cand ? sc2 : qnan();
      stop[k] = cand ? sl : qnan();
    }
    put_codes(A.status + orow, tb, T, vbytes, stt);
    if (A.score) store_lines<TG::K>(A.score + orow, tb, T, vout, score, whole);
    if (A.stop) store_lines<TG::K>(A.stop + orow, tb, T, vout, stop, whole);

    if (t0 + TG::TT >= T) break;
    __syncthreads();   // every read of this tile's ring is done
    if (pb >= TG::TT) {   // halo of the next tile: the last TG::H positions
#pragma unroll
      for (int k = 0; k < TG::K; ++k) {
        const int a = TG::slot(pb + k), d = TG::slot(pb + k - TG::TT);
        sH[d] = sH[a];
        sC[d] = sC[a];
        sV[d] = sV[a];
        if (QV) sQ[d] = sQ[a];
      }
    }
    if (tid == TG::NT - 1) {
      sEC[0] = ewy[0];   // (a serial row: unused)
      sEC[1] = ewy[1];
    }
    if (tid == 0) {
      sBad = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sTE[0][j] = sTE[TG::NW][j];
        sTP[0][j] = sTP[TG::NW][j];
        sTS[0][j] = sTS[TG::NW][j];
      }
    }
    __syncthreads();
  }
}

}  // namespace bq

extern "C" void bq_top_gainer_default_params(bq_top_gainer_params* p) {
  if (!p) return;
  // TopGainerEarlyMomentum's class attributes (:42-57, :64-66)
  p->lookback_high = 48;
  p->volume_window = 32;
  p->min_history = 56;
  p->full_extension_bars = 96;
  p->min_candle_return = 0.01;
  p->max_candle_return = 0.10;
  p->min_return_1h = 0.05;
  p->min_return_2h = 0.08;
  p->min_return_6h = 0.07;
  p->max_return_1h = 0.20;
  p->max_extension = 0.50;
  p->min_short_extension_cap = 0.25;
  p->min_volume_ratio = 1.75;
  p->min_range_position = 0.75;
  p->max_upper_wick = 0.30;
  p->atr_stop_mult = 2.2;
  p->min_stop_loss_pct = 1.5;
  p->max_stop_loss_pct = 2.0;
}

namespace {
// pandas: alpha = 1 / (1 + com), com = (span - 1) / 2
void tg_ewm_consts(bq::TgEwm& E, double span) {
  E.alpha = 1.0 / (1.0 + (span - 1.0) / 2.0);
  E.om = 1.0 - E.alpha;
  E.den = E.om + E.alpha;
  E.div = E.den != 1.0;
  E.la = E.om / E.den;
  E.lb = E.alpha / E.den;
  double a4 = E.la * E.la;
  a4 *= a4;   // la^4
  E.apow[0] = a4;
  for (int j = 1; j < 8; ++j) E.apow[j] = E.apow[j - 1] * E.apow[j - 1];
  E.mw = E.apow[6];   // la^(4 * 64)
}

template <bool QV>
void tg_launch(const bq::TgArgs& A, int64_t S, int vflags, hipStream_t stream) {
  using namespace bq;
  if (A.p.lookback_high == 48 && A.p.volume_window == 32)   // the class attributes
    hipLaunchKernelGGL((top_gainer_kernel<QV, 48, 32>), dim3((unsigned)S), dim3(TG::NT), 0, stream, A, vflags);
  else
    hipLaunchKernelGGL((top_gainer_kernel<QV>), dim3((unsigned)S), dim3(TG::NT), 0, stream, A, vflags);
}
}  // namespace

extern "C" int bq_top_gainer_entry(const double* open, const double* high, const double* low, const double* close,
                                   const double* volume, int64_t ld_in, const double* quote_volume, int64_t ld_qv,
                                   const double* atr, int64_t ld_atr, const uint8_t* risk_ok, int64_t ld_risk,
                                   const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T,
                                   const bq_top_gainer_params* params, uint8_t* status, uint8_t* entry, double* score,
                                   double* stop_loss_pct, double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!open || !high || !low || !close || !volume || !status || !entry || S < 0 || T < 0 || ld_in < T ||
      ld_out < T || (quote_volume && ld_qv < T) || (atr && ld_atr < T) || (risk_ok && ld_risk < T) ||
      T > 0x7fffffff - 2 * TG::TT || S > 0x7fffffff)
    return BQ_EINVAL;
  TgArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_top_gainer_default_params(&A.p);
  const int H = BQ_TGE_MAX_LOOKBACK;
  if (A.p.lookback_high < 1 || A.p.lookback_high > H || A.p.volume_window < 1 || A.p.volume_window > H ||
      A.p.full_extension_bars < 1 || A.p.full_extension_bars > H)
    return BQ_EINVAL;   // the windows stay inside the ring's halo
  if (A.p.min_history < 25) return BQ_EINVAL;   // the returns reach t - 24
  if (S == 0 || T == 0) return BQ_OK;
  A.open = open;
  A.high = high;
  A.low = low;
  A.close = close;
  A.volume = volume;
  A.qv = quote_volume;
  A.atr = atr;
  A.risk = risk_ok;
  A.lens = lens;
  A.first = first_t;
  A.ld_in = ld_in;
  A.ld_qv = ld_qv;
  A.ld_atr = ld_atr;
  A.ld_risk = ld_risk;
  A.ld_out = ld_out;
  A.T = (int)T;
  tg_ewm_consts(A.ew[0], 20.0);   // close.ewm(span=20, adjust=False) (:153)
  tg_ewm_consts(A.ew[1], 50.0);   // close.ewm(span=50, adjust=False) (:154)
  A.status = status;
  A.entry = entry;
  A.score = score;
  A.stop = stop_loss_pct;
  const double* outs[BQ_TGE_NVALUES + 2];
  for (int k = 0; k < BQ_TGE_NVALUES; ++k) outs[k] = A.val[k] = values ? values[k] : nullptr;
  outs[BQ_TGE_NVALUES] = score;
  outs[BQ_TGE_NVALUES + 1] = stop_loss_pct;
  const double* ins[5] = {open, high, low, close, volume};
  const uint8_t* codes[2] = {status, entry};
  const int vflags = (vec_rows(ins, 5, ld_in) ? TG_VIN : 0) | (vec_rows(&quote_volume, 1, ld_qv) ? TG_VQV : 0) |
                     (vec_rows(&atr, 1, ld_atr) ? TG_VATR : 0) |
                     (vec_rows(outs, BQ_TGE_NVALUES + 2, ld_out) ? TG_VOUT : 0) |
                     (vec_bytes(codes, 2, ld_out) ? TG_VBYTES : 0);
  if (quote_volume) tg_launch<true>(A, S, vflags, (hipStream_t)stream);
  else tg_launch<false>(A, S, vflags, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
