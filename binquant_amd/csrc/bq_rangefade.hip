// RangeBbRsiMeanReversion.signal() replayed over a [S][T] panel of 15m frames
// (gfx950; strategies/range_bb_rsi_mean_reversion.py:202-274): the frame and
// null gate, the eleven steps of regime_routing, _compute_adx and the ADX cut,
// _compute_zscore, _resolve_entry's two band-rejection candle tests with their
// RSI and z-score confirmation, and local_score. Column t of row s = the method
// on the message whose frame is df_15m.iloc[first_t[s]:t + 1] (the rule table:
// include/binquant_amd.h). The strategy keeps no cooldown entry: no state.
//
// range_fade_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. <FEAT = true> forms adx and zscore over the frame starting at first_t.
//      The windows are finite, so a replayed candle reads no further back than
//      the step before its own: the features are formed from the step before
//      from_t's on, which loads high / low / close only. The frame gate and
//      the routing come first; a step none of whose candles gets as far as the
//      ADX cut forms only the per-candle series and dx (the next step's
//      windows read them) and leaves the second-level and z-score walks out.
//      - _compute_adx (:101-130): diff() and shift(1) cross the step edge
//        through lane 63's carried high / low / close; the frame's first row has
//        no previous candle (+DM = -DM = 0.0, the skip-NaN max leaves high -
//        low). The three rolling(w, min_periods = w) sums and the second-level
//        rolling(w).mean() of dx are direct sums over the window's w lanes: the
//        series is shifted one lane per term (DPP wave_shr:1, lane 0 fed with
//        the previous step's lane 64 - k at the k-th term), so a window reads
//        this step's registers and the previous step's — tr, +DM, -DM and dx of
//        the previous step are the carried register set. Two terms per loop
//        trip; the moves are convergent, so the compiler does not unroll the
//        walks, and an instance for the reference's windows that unrolls them
//        completely was dropped (181 VGPRs, 2 waves / SIMD). Every term is
//        >= 0, so a plain sum of w <= 32 terms is within (w - 1) 2^-53
//        relative of the exact sum: no cancellation, no prefix that grows with
//        T, nothing to compensate (the double-double prefix of §4.23 buys
//        accuracy only where terms cancel). dx is 0.0, not NaN, wherever the
//        sums are not ready or the DI total is 0 or NaN (fillna(0.0)), so the
//        mean is finite from frame row w - 1 on and includes those zeros; adx
//        is 100.0 only while the frame is shorter than the window. A NaN true
//        range is excluded and counted through the step's and the previous
//        step's ballots (dx = 0.0 while a window holds it).
//      - _compute_zscore (:132-138), zscore_kernel's rules (bq_signals.hip):
//        the window's closes shifted by a finite lane-local reference, here the
//        candle's own close c: s1 = sum (x - c), s2 = sum (x - c)^2 by the same
//        lane shifts, var = (s2 - s1^2 / w) / w, z = (-s1 / w) / sqrt(var). A
//        window of one repeated value has every x - c exactly 0: std exactly 0
//        and z exactly 0.0. z is 0.0 during the warm-up and while the window
//        holds a NaN close (ballots, as above).
//      <FEAT = false> reads the two columns instead and is point-wise.
//   2. the null gate's tail(5) at lanes 0-3 reads the previous step's last four
//      null flags: its ballot is carried (the first replayed step of a row
//      that starts past candle 0 forms it from four candles' loads).
//   3. the gates are point-wise, in the method's order and operation order;
//      Python's min / max are selects.
//   9 x 8 B in (+ the context rows, L2-resident, + 19 B of symbol snapshot
//   where it is per candle, + 16 B with the features given) and 1 + 4 x 8 B out
//   per candle; LDS 0, no atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3; make resource-usage): <FEAT =
//   true> 114 VGPRs, 99 SGPRs, 4 waves / SIMD; <FEAT = false> 94 VGPRs, 94
//   SGPRs, 5 waves / SIMD. No spills, scratch 0, LDS 0 in both.
//
// Domain: prices finite or NaN inside the frame (+-inf in a price is outside
// this entry's contract and untested).
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

constexpr int RF_TAIL = 5;            // df[required_cols].tail(5) (:212)

struct RfArgs {
  const double *open, *high, *low, *close, *volume, *rsi, *bbu, *bbm, *bbl;
  const double* feat[BQ_RF_NFEATURES];
  const double* ctx;
  const uint8_t* ctx_ok;
  const uint8_t *sym_ok, *sym_regime, *sym_transition;
  const double *sym_atr, *sym_bbw;
  const int64_t *lens, *first, *from;
  int64_t ld_px, ld_rsi, ld_bb, ld_ft, ld_sym, ld_out, S;
  int T, ctx_T, ld_ctx, omask;
  bq_range_fade_params p;
  uint8_t* status;
  double* val[BQ_RF_NVALUES];
};

struct RfStep {
  double o, h, l, c, v, rsi, bbu, bbm, bbl;
  double f[BQ_RF_NFEATURES];
};

// the k-th move of one lane to the right along the 128 candles (previous step q, this step x): x's lane i receives
// lane i - 1, lane 0 the previous step's lane 64 - k
// (without bound_ctrl a lane that has no source, lane 0, keeps the DPP move's old value: the feed)
__device__ __forceinline__ void rf_shift(double& x, double q, int k) {
  const int ilo = __builtin_amdgcn_readlane(__double2loint(q), WAVE - k);
  const int ihi = __builtin_amdgcn_readlane(__double2hiint(q), WAVE - k);
  const int lo = __builtin_amdgcn_update_dpp(ilo, __double2loint(x), DPP_WAVE_SHR1, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(ihi, __double2hiint(x), DPP_WAVE_SHR1, 0xF, 0xF, false);
  x = __hiloint2double(hi, lo);
}

// f(k) for the window's terms k = 1 .. w - 1, two per trip (the lane moves are convergent, so the compiler does not
// unroll the walk itself; a pair per trip spares the register copies at the loop's back edge)
template <typename F>
__device__ __forceinline__ void rf_walk(int w, F&& f) {
  int k = 1;
  for (; k + 1 < w; k += 2) {
    f(k);
    f(k + 1);
  }
  if (k < w) f(k);
}

template <bool FEAT>
__global__ __launch_bounds__(RP_NT) void range_fade_kernel(const RfArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const double* __restrict__ op = A.open + s * A.ld_px;
  const double* __restrict__ hp = A.high + s * A.ld_px;
  const double* __restrict__ lp = A.low + s * A.ld_px;
  const double* __restrict__ cp = A.close + s * A.ld_px;
  const double* __restrict__ vp = A.volume + s * A.ld_px;
  const double* __restrict__ rp = A.rsi + s * A.ld_rsi;
  const double* __restrict__ bup = A.bbu + s * A.ld_bb;
  const double* __restrict__ bmp = A.bbm + s * A.ld_bb;
  const double* __restrict__ blp = A.bbl + s * A.ld_bb;
  ReplayOut<RfArgs, BQ_RF_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_RF_NVALUES; ++k) O.set(k, A.val[k]);

  // one step's columns, candle tb + lane (NaN past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    RfStep x;
    x.o = in ? op[u] : qnan();
    x.h = in ? hp[u] : qnan();
    x.l = in ? lp[u] : qnan();
    x.c = in ? cp[u] : qnan();
    x.v = in ? vp[u] : qnan();
    x.rsi = in ? rp[u] : qnan();
    x.bbu = in ? bup[u] : qnan();
    x.bbm = in ? bmp[u] : qnan();
    x.bbl = in ? blp[u] : qnan();
#pragma unroll
    for (int k = 0; k < BQ_RF_NFEATURES; ++k) {
      if (FEAT) {
        x.f[k] = 0.0;
      } else {
        const double* fp = kernarg<RfArgs>()->feat[k] + s * kernarg<RfArgs>()->ld_ft;
        x.f[k] = in ? fp[u] : qnan();
      }
    }
    return x;
  };

  // the first step the features are formed on: the windows are finite (2 adx_window - 1 <= 63 candles for the ADX,
  // zscore_window <= 64 closes), so a replayed candle reads no further back than the step before its own
  const int b0 = R.b0(), e0 = R.e0();
  const int f0 = b0 - WAVE > e0 ? b0 - WAVE : e0;
  const bool any = R.any();

  // ---- the in-pass features' state: lane 63's candle, the previous step's series and missing-value ballots
  double h_carry = qnan(), l_carry = qnan(), c_carry = qnan();
  double tr_prev = 0.0, pd_prev = 0.0, md_prev = 0.0, dx_prev = 0.0, cl_prev = qnan();
  uint64_t tb_prev = 0, cb_prev = 0;
  uint64_t null_prev = 0;   // the previous step's null flags (the gate's tail(5))

  // candles t0 .. t0 + 63: adx and zscore (every lane executes it; called once for every step from f0 on, in order).
  // need (wave-uniform): a candle of the step gets as far as the ADX cut; without one only the per-candle series and
  // dx, which the next step's windows read, are formed
  auto feat_step = [&](double h, double l, double c, int t0, bool need, double (&f)[BQ_RF_NFEATURES]) {
    const int t = t0 + lane;
    const int r = t - first;   // the frame's row
    const Karg<RfArgs> K = kernarg<RfArgs>();
    const int W = K->p.adx_window, WZ = K->p.zscore_window;
    double ph = dpp_f64<DPP_WAVE_SHR1>(h), pl = dpp_f64<DPP_WAVE_SHR1>(l), pc = dpp_f64<DPP_WAVE_SHR1>(c);
    if (lane == 0) {
      ph = h_carry;
      pl = l_carry;
      pc = c_carry;
    }
    h_carry = readlane_f64(h, WAVE - 1);
    l_carry = readlane_f64(l, WAVE - 1);
    c_carry = readlane_f64(c, WAVE - 1);
    asm volatile("" : "+v"(h_carry), "+v"(l_carry), "+v"(c_carry));
    if (r <= 0) ph = pl = pc = qnan();   // diff() / shift(1): NaN on the frame's first row
    // :106-117 (a NaN difference fails both compares: 0.0; the max skips NaN)
    const double hd = h - ph, ld = -(l - pl);
    double pd = (hd > ld && hd > 0.0) ? hd : 0.0;
    double md = (ld > hd && ld > 0.0) ? ld : 0.0;
    double tr = true_range(h, l, pc);
    const bool trbad = r >= 0 && tr != tr;
    if (r < 0 || trbad) tr = 0.0;
    if (r < 0) pd = md = 0.0;
    const uint64_t TB = __ballot(trbad);

    // :119-121: the three sums over candles t - W + 1 .. t
    double st = tr, sp = pd, sm = md;
    {
      double xt = tr, xp = pd, xm = md;
      rf_walk(W, [&](int k) {
        rf_shift(xt, tr_prev, k);
        rf_shift(xp, pd_prev, k);
        rf_shift(xm, md_prev, k);
        st += xt;
        sp += xp;
        sm += xm;
      });
    }
    const bool ready = r + 1 >= W;   // min_periods = window
    const double asum = (ready && !window_hit(TB, tb_prev, W, lane)) ? st : qnan();
    const double pdi = 100.0 * (ready ? sp : qnan()) / asum, mdi = 100.0 * (ready ? sm : qnan()) / asum;   // :120-121
    const double tot = pdi + mdi;
    double dx = tot != 0.0 ? 100.0 * fabs(pdi - mdi) / tot : qnan();   // :123-127
    if (dx != dx) dx = 0.0;                                            // fillna(0.0)
    double sd = dx;
    if (need) {
      double x = dx;
      rf_walk(W, [&](int k) {
        rf_shift(x, dx_prev, k);
        sd += x;
      });
    }
    f[BQ_RF_V_ADX] = ready ? sd / (double)W : 100.0;   // :128-129
    tr_prev = tr;
    pd_prev = pd;
    md_prev = md;
    dx_prev = dx;
    tb_prev = TB;

    // :132-138
    const uint64_t CB = __ballot(r >= 0 && c != c);
    double s1 = 0.0, s2 = 0.0;
    if (need) {
      double x = c;
      rf_walk(WZ, [&](int k) {
        rf_shift(x, cl_prev, k);
        const double d = x - c;
        s1 += d;
        s2 = fma(d, d, s2);
      });
    }
    double z = 0.0;
    if (r + 1 >= WZ && !window_hit(CB, cb_prev, WZ, lane)) {
      const double w = (double)WZ;
      const double var = (s2 - (s1 * s1) / w) / w;
      const double sdev = var > 0.0 ? sqrt(var) : 0.0;
      if (sdev > 0.0) z = (-(s1 / w)) / sdev;   // close - mean = -(s1 / w) with the candle's own close as the reference
    }
    f[BQ_RF_V_ZSCORE] = z;
    cl_prev = c;
    cb_prev = CB;
  };

  RfStep nxt = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) O.no_frame(t0, BQ_RF_NO_FRAME);
      if (FEAT && any && t0 >= f0 && t0 < b0) {   // the step a replayed candle's windows reach back into
        double f[BQ_RF_NFEATURES];
        const bool in = t < T;
        feat_step(in ? hp[t] : qnan(), in ? lp[t] : qnan(), in ? cp[t] : qnan(), t0, false, f);
      }
      continue;
    }
    if (t0 == b0) {
      nxt = load_step(t0);
      if (t0 > 0) {   // the null flags of candles t0 - 4 .. t0 - 1, at lanes 60 .. 63 of the previous step's ballot
        const int u = t0 - WAVE + lane;
        bool nul = false;
        if (lane >= WAVE - (RF_TAIL - 1) && u >= first) {
          const double a = op[u], b = hp[u], c = lp[u], d = cp[u], e = vp[u], g = rp[u];
          nul = a != a || b != b || c != c || d != d || e != e || g != g;
        }
        null_prev = __ballot(nul);
      }
    }
    const RfStep cur = nxt;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's arithmetic
    const bool valid = t >= from && t < len;
    const Karg<RfArgs> K = kernarg<RfArgs>();
    const auto& P = K->p;

    // :212: the frame's length, and isnull (NaN only) over the last min(5, rows) candles of the six columns
    const bool nul = t >= first && (cur.o != cur.o || cur.h != cur.h || cur.l != cur.l || cur.c != cur.c ||
                                    cur.rsi != cur.rsi || cur.v != cur.v);
    const uint64_t NB = __ballot(nul);
    const bool short_frame = t + 1 - first < P.min_candles || window_hit(NB, null_prev, RF_TAIL, lane);
    null_prev = NB;

    // the context and the symbol's snapshot entry at the candle's message
    double cx[3];
    const bool cok = ctx_load(K, ctx_index(K, t, T), cx);
    const double trans = cx[0], stress = cx[1], regime = cx[2];
    bool sok = false;
    double satr = 0.0, sbbw = 0.0;
    int sreg = BQ_RF_NONE, strans = BQ_RF_NONE;
    if (K->sym_ok) {   // wave-uniform
      const int64_t si = sym_index(K, s, t, T);
      sok = K->sym_ok[si] != 0;
      satr = K->sym_atr[si];
      sbbw = K->sym_bbw[si];
      sreg = K->sym_regime[si];
      strans = K->sym_transition[si];
    }

    // the frame gate and regime_routing (:212, :71-97); a candle that passes gets as far as the ADX cut
    int st = BQ_RF_EMIT;
    if (!valid) st = BQ_RF_NO_FRAME;
    else if (short_frame) st = BQ_RF_NOT_ENOUGH_DATA;
    else if (!cok) st = BQ_RF_NO_CONTEXT;                                        // :71
    else if (trans != 0.0) st = BQ_RF_TRANSITIONING;                             // :73
    else if (stress >= P.max_market_stress) st = BQ_RF_STRESS;                   // :75
    else if (regime == (double)BQ_RF_NONE) st = BQ_RF_NO_REGIME;                 // :77
    else if (regime != (double)BQ_RF_REGIME_RANGE) st = BQ_RF_REGIME_NOT_RANGE;  // :79
    else if (!sok) st = BQ_RF_NO_SYMBOL;                                         // :81
    else if (sreg != BQ_RF_REGIME_RANGE) st = BQ_RF_SYMBOL_NOT_RANGE;            // :83
    else if (strans == BQ_RF_TRANSITION_BREAKOUT_UP || strans == BQ_RF_TRANSITION_BREAKDOWN ||
             strans == BQ_RF_TRANSITION_VOLATILITY_EXPANSION)
      st = BQ_RF_SYMBOL_TRANSITION;                                              // :85
    else if (satr > P.max_symbol_atr_pct) st = BQ_RF_SYMBOL_ATR;                 // :94
    else if (sbbw > P.max_symbol_bb_width) st = BQ_RF_SYMBOL_BB_WIDTH;           // :96

    double f[BQ_RF_NFEATURES];
    if (FEAT) {
      feat_step(cur.h, cur.l, cur.c, t0, __ballot(st == BQ_RF_EMIT) != 0, f);
    } else {
#pragma unroll
      for (int k = 0; k < BQ_RF_NFEATURES; ++k) f[k] = cur.f[k];
    }
    const double adx = f[BQ_RF_V_ADX], z = f[BQ_RF_V_ZSCORE];

    // :140-166 (compares in the method's direction: a NaN fails)
    const double range = cur.h - cur.l;
    const bool norange = range <= 0.0;
    const double closepos = (cur.c - cur.l) / range;
    const bool bull = !norange && cur.l <= cur.bbl * (1.0 + P.band_touch_tolerance) && cur.c > cur.o &&
                      (py_min(cur.o, cur.c) - cur.l) / range >= P.min_rejection_wick_frac &&
                      closepos >= P.long_close_position_min;
    const bool bear = !norange && cur.h >= cur.bbu * (1.0 - P.band_touch_tolerance) && cur.c < cur.o &&
                      (cur.h - py_max(cur.o, cur.c)) / range >= P.min_rejection_wick_frac &&
                      closepos <= P.short_close_position_max;
    // :180-194 (current_price is the candle's close)
    const bool lng = cur.c <= cur.bbm && cur.rsi <= P.long_rsi_max && z <= P.long_zscore_max && bull;
    const bool sht = cur.c >= cur.bbm && cur.rsi >= P.short_rsi_min && z >= P.short_zscore_min && bear;

    if (st == BQ_RF_EMIT) {
      if (adx > P.adx_max) st = BQ_RF_ADX_TOO_HIGH;      // :230
      else if (!lng && !sht) st = BQ_RF_NO_SETUP;       // :243
    }

    // :264-274, unrounded, in the method's operation order
    const double rpart = lng ? py_max(0.0, (P.long_rsi_max - cur.rsi) / P.long_rsi_max)
                             : py_max(0.0, (cur.rsi - P.short_rsi_min) / 35.0);
    const double score = ((1.0 + py_min(fabs(z) / 3.0, 1.0) * 0.35) +
                          py_max(0.0, (P.adx_max - adx) / P.adx_max) * 0.25) + rpart * 0.25;

    if (t < T) {
      O.st[t0] = (uint8_t)st;
      const bool emit = st == BQ_RF_EMIT;
      if (O.has(BQ_RF_V_ADX)) O.val[BQ_RF_V_ADX][t0] = (emit || st >= BQ_RF_ADX_TOO_HIGH) ? adx : qnan();
      if (O.has(BQ_RF_V_ZSCORE)) O.val[BQ_RF_V_ZSCORE][t0] = (emit || st >= BQ_RF_NO_SETUP) ? z : qnan();
      if (O.has(BQ_RF_V_DIRECTION))
        O.val[BQ_RF_V_DIRECTION][t0] = emit ? (lng ? (double)BQ_DIR_LONG : (double)BQ_DIR_SHORT) : qnan();
      if (O.has(BQ_RF_V_SCORE)) O.val[BQ_RF_V_SCORE][t0] = emit ? score : qnan();
    }
  }
}

}  // namespace bq

extern "C" void bq_range_fade_default_params(bq_range_fade_params* p) {
  if (!p) return;
  // RangeBbRsiMeanReversion's class attributes (range_bb_rsi_mean_reversion.py:37-51)
  p->min_candles = 40;
  p->adx_window = 14;
  p->zscore_window = 20;
  p->reserved = 0;
  p->adx_max = 32.0;
  p->long_rsi_max = 35.0;
  p->short_rsi_min = 65.0;
  p->long_zscore_max = -2.0;
  p->short_zscore_min = 2.0;
  p->band_touch_tolerance = 0.002;
  p->max_market_stress = 0.35;
  p->max_symbol_atr_pct = 0.04;
  p->max_symbol_bb_width = 0.08;
  p->min_rejection_wick_frac = 0.30;
  p->long_close_position_min = 0.55;
  p->short_close_position_max = 0.45;
}

extern "C" int bq_range_fade_replay(const double* open, const double* high, const double* low, const double* close,
                                    const double* volume, int64_t ld_px, const double* rsi, int64_t ld_rsi,
                                    const double* bb_upper, const double* bb_mid, const double* bb_lower,
                                    int64_t ld_bb, const double* const* features, int64_t ld_ft, const double* ctx,
                                    int64_t ld_ctx, const uint8_t* ctx_ok, int64_t ctx_T, const uint8_t* sym_ok,
                                    const uint8_t* sym_regime, const uint8_t* sym_transition,
                                    const double* sym_atr_pct, const double* sym_bb_width, int64_t ld_sym,
                                    const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S,
                                    int64_t T, const bq_range_fade_params* params, uint8_t* status,
                                    double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!open || !high || !low || !close || !volume || !rsi || !bb_upper || !bb_mid || !bb_lower || !ctx || !status ||
      S < 0 || T < 0 || ld_px < T || ld_rsi < T || ld_bb < T || ld_out < T || (features && ld_ft < T) ||
      (ld_sym != 0 && ld_sym < T) || (ctx_T != 1 && ctx_T != T) || ld_ctx < ctx_T || ld_ctx > 0x1fffffff ||
      T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  if (sym_ok && (!sym_regime || !sym_transition || !sym_atr_pct || !sym_bb_width)) return BQ_EINVAL;
  if (features)
    for (int k = 0; k < BQ_RF_NFEATURES; ++k)
      if (!features[k]) return BQ_EINVAL;
  RfArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_range_fade_default_params(&A.p);
  const bq_range_fade_params& p = A.p;
  if (!all_finite({p.adx_max, p.long_rsi_max, p.short_rsi_min, p.long_zscore_max, p.short_zscore_min,
                   p.band_touch_tolerance, p.max_market_stress, p.max_symbol_atr_pct, p.max_symbol_bb_width,
                   p.min_rejection_wick_frac, p.long_close_position_min, p.short_close_position_max}))
    return BQ_EINVAL;
  if (p.min_candles < 1 || p.adx_window < 1 || p.adx_window > BQ_RF_MAX_ADX_WINDOW || p.zscore_window < 1 ||
      p.zscore_window > BQ_RF_MAX_ZSCORE_WINDOW || p.adx_max == 0.0 || p.long_rsi_max == 0.0)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.open = open;
  A.high = high;
  A.low = low;
  A.close = close;
  A.volume = volume;
  A.rsi = rsi;
  A.bbu = bb_upper;
  A.bbm = bb_mid;
  A.bbl = bb_lower;
  for (int k = 0; k < BQ_RF_NFEATURES; ++k) A.feat[k] = features ? features[k] : nullptr;
  A.ctx = ctx;
  A.ctx_ok = ctx_ok;
  A.sym_ok = sym_ok;
  A.sym_regime = sym_regime;
  A.sym_transition = sym_transition;
  A.sym_atr = sym_atr_pct;
  A.sym_bbw = sym_bb_width;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_px = ld_px;
  A.ld_rsi = ld_rsi;
  A.ld_bb = ld_bb;
  A.ld_ft = ld_ft;
  A.ld_sym = ld_sym;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.ctx_T = (int)ctx_T;
  A.ld_ctx = (int)ld_ctx;
  A.status = status;
  replay_values(A.val, A.omask, values);
  const dim3 grid((unsigned)blocks), block(RP_NT);
  hipStream_t st = (hipStream_t)stream;
  if (features) hipLaunchKernelGGL((range_fade_kernel<false>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((range_fade_kernel<true>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
