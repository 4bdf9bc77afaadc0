// MeanReversionFade.signal() replayed over a [S][T] panel of 15m frames (gfx950;
// strategies/mean_reversion_fade.py:224-300): the Wilder RSI and its hook, the
// 20-bar means of volume and ATR, the EMA 20 / 50 trend score, the not-ready
// gate, _resolve_entry's five ordered checks, the trend ceiling, the SHORT
// branch of _risk_profile_allows, the once-per-candle test and the stop-loss
// cap. Column t of row s = the method on the message whose frame is
// df_15m.iloc[first_t[s]:t + 1], after the messages of all earlier candles of
// the row (the rule table: include/binquant_amd.h). _resolve_entry only ever
// returns Position.short: the LONG branch of _risk_profile_allows (:185-198)
// cannot be reached and is not built.
//
// mean_reversion_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. <FEAT = true> forms the five features over the frame starting at
//      first_t; steps between first_t's and from_t's load close / volume / atr
//      only.
//      - _rsi (:88-109): diff() across the step edge (lane 63's close is
//        carried), clip, and the two ewm(alpha = 1 / 14, min_periods = 14,
//        adjust=False) means through bq_replay.h's ewm_step. A flat stretch
//        scans zeros to exactly 0 + 0 -> 50.0; a loss-free rally leaves the
//        loss mean exactly 0 -> 100 g / g. previous_rsi is the lane to the
//        left, or the previous step's lane 63.
//      - _trend_score (:149-155): the same ewm_step call's ewm(span = 20 / 50)
//        (four series over three constant sets; a NaN or infinite close
//        inside the frame turns all four serial).
//      - rolling(20).mean() of volume and ATR: a double-double wave prefix
//        per step; the window sum is prefix[t] - prefix[t - w], where a window
//        that reaches into the previous step adds that step's total minus its
//        prefix (both kept in registers: two lane reads). The prefix restarts
//        every step, so nothing grows with T. Missing values (NaN; +-inf as
//        pandas' windows see it) count through the step's and the previous
//        step's ballots; min_periods = window.
//      <FEAT = false> reads the five columns instead and is point-wise.
//   2. the gates are point-wise, in the method's order and operation order.
//   3. the once-per-candle test needs no serial walk: open_time is strictly
//      ascending, so the row's entry can equal open_time[t] only while it is
//      still the entry the call started with, i.e. while no earlier candle of
//      the call has emitted (a ballot prefix plus one wave-uniform flag). The
//      state after the call is the last emitting candle's open time.
//   8 x 8 B in (+ the context rows, L2-resident, + 18 B of symbol snapshot
//   where it is per candle) and 1 + 7 x 8 B out per candle; LDS only as the
//   lane-read crossbar (no allocation), no atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3; make resource-usage): <FEAT =
//   true> 160 VGPRs, 106 SGPRs, 3 waves / SIMD; <FEAT = false> 94 VGPRs, 98
//   SGPRs, 5 waves / SIMD. No spills, scratch 0, LDS 0 in both.
//
// Domain: open_time strictly ascending within [first_t, lens); volume and atr
// finite or NaN inside the frame.
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// the scanned series: gain and loss (Wilder's set, differences: seeded at first_t + 1, min_periods = rsi_window),
// ema_fast and ema_slow of close (seeded at first_t); a missing close turns the row serial
struct MrSeries {
  static constexpr int NE = 4, NK = 3, SWITCH = 2;
  static constexpr int set(int e) { return e < 2 ? 0 : e - 1; }
  static constexpr int seed(int e) { return e < 2 ? 1 : 0; }
  static constexpr bool min_periods(int e) { return e < 2; }
};
constexpr int MR_NE = MrSeries::NE;

struct MrArgs {
  const double *open, *high, *low, *close, *volume, *atr, *bb;
  const int64_t* ot;
  const double* feat[BQ_MR_NFEATURES];
  const double* ctx;
  const uint8_t* ctx_ok;
  const uint8_t *sym_ok, *sym_regime, *sym_transition;
  const double *sym_atr, *sym_trend;
  const int64_t *lens, *first, *from;
  int64_t ld_px, ld_atr, ld_bb, ld_ot, ld_ft, ld_sym, ld_out, S;
  int T, ctx_T, ld_ctx, omask;
  bq_mean_reversion_params p;
  Ewm ew[3];   // Wilder (gain and loss), span ema_fast, span ema_slow
  uint8_t* st_has;
  int64_t* st_last;
  uint8_t* status;
  double* val[BQ_MR_NVALUES];
};

struct MrStep {
  double o, h, l, c, v, a, bb;
  double f[BQ_MR_NFEATURES];
  int64_t ot;
};

template <bool FEAT>
__global__ __launch_bounds__(RP_NT) void mean_reversion_kernel(const MrArgs A) {
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
  const double* __restrict__ ap = A.atr + s * A.ld_atr;
  const double* __restrict__ bp = A.bb + s * A.ld_bb;
  const int64_t* __restrict__ otp = A.ot + s * A.ld_ot;
  ReplayOut<MrArgs, BQ_MR_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_MR_NVALUES; ++k) O.set(k, A.val[k]);

  // the row's entry as the call found it, and what this call emitted: wave-uniform
  const bool has0 = A.st_has && A.st_has[s] != 0;
  const int64_t last0 = has0 ? A.st_last[s] : 0;
  bool emitted = false;
  int64_t last_emit = 0;

  // one step's columns, candle tb + lane (NaN / 0 past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    MrStep x;
    x.o = in ? op[u] : qnan();
    x.h = in ? hp[u] : qnan();
    x.l = in ? lp[u] : qnan();
    x.c = in ? cp[u] : qnan();
    x.v = in ? vp[u] : qnan();
    x.a = in ? ap[u] : qnan();
    x.bb = in ? bp[u] : qnan();
#pragma unroll
    for (int k = 0; k < BQ_MR_NFEATURES; ++k) {
      if (FEAT) {
        x.f[k] = 0.0;
      } else {
        const double* fp = kernarg<MrArgs>()->feat[k] + s * kernarg<MrArgs>()->ld_ft;
        x.f[k] = in ? fp[u] : qnan();
      }
    }
    x.ot = in ? otp[u] : 0;
    return x;
  };

  const int b0 = R.b0(), e0 = R.e0();
  const bool any = R.any();

  // ---- the in-pass features' state
  EwmState<MrSeries::NE, MrSeries::NK> ES;
  ewm_init<MrSeries>(ES, A.ew, lane, FEAT);
  double close_carry = qnan(), rsi_carry = qnan();
  dd pv_prev = {0.0, 0.0}, pa_prev = {0.0, 0.0};   // the previous step's prefixes of volume / atr
  uint64_t bv_prev = 0, ba_prev = 0;               // and its missing-value ballots

  // rolling(w).mean() of candles t0 .. t0 + 63 (every lane executes it)
  auto window_mean = [&](double x, int w, int t0, dd& pprev, uint64_t& bprev) {
    const int t = t0 + lane;
    const bool ok = win_ok(x);
    const dd P = wave_scan_dd_dpp(dd{ok ? x : 0.0, 0.0}, lane);
    const uint64_t NB = __ballot(!ok);
    const int j = lane - w;   // the newest candle before the window
    const int src = j & (WAVE - 1);
    const dd a = {__shfl(P.hi, src, WAVE), __shfl(P.lo, src, WAVE)};
    const dd b = {__shfl(pprev.hi, src, WAVE), __shfl(pprev.lo, src, WAVE)};
    const dd tot = {readlane_f64(pprev.hi, WAVE - 1), readlane_f64(pprev.lo, WAVE - 1)};
    const dd in_step = dd_add(P, dd{-a.hi, -a.lo});
    const dd across = dd_add(P, dd_add(tot, dd{-b.hi, -b.lo}));
    const dd sum = j >= 0 ? in_step : across;
    const bool bad = window_hit(NB, bprev, w, lane);
    pprev = P;
    bprev = NB;
    return (t + 1 - first >= w && !bad) ? dd_round(sum) / (double)w : qnan();
  };

  // candles t0 .. t0 + 63: rsi, previous_rsi, volume_ma, atr_ma, trend_score into f (every lane executes it;
  // called once for every step from e0 on, in order)
  auto feat_step = [&](double c, double v, double a, int t0, double (&f)[BQ_MR_NFEATURES]) {
    const int t = t0 + lane;
    const Karg<MrArgs> K = kernarg<MrArgs>();
    const int W = K->p.rsi_window;
    double pc = dpp_f64<DPP_WAVE_SHR1>(c);
    if (lane == 0) pc = close_carry;
    close_carry = readlane_f64(c, WAVE - 1);
    asm volatile("" : "+v"(close_carry));
    const double d = t > first ? c - pc : qnan();   // diff(): NaN on the frame's first row
    double x[MR_NE], y[MR_NE];
    x[0] = win_val(d != d ? d : (d > 0.0 ? d : 0.0));    // clip(lower=0) keeps NaN; ewm: +-inf is missing
    x[1] = win_val(d != d ? d : (d < 0.0 ? -d : 0.0));   // -clip(upper=0)
    x[2] = x[3] = win_val(c);
    ewm_step<MrSeries>(ES, K->ew, x, t0, lane, first, len, W, y);
    const double den = y[0] + y[1];
    double rsi = den != 0.0 ? (100.0 * y[0]) / den : 50.0;   // .where(denom != 0, 50.0): a NaN denominator stays NaN
    if (t < first) rsi = qnan();
    double prsi = dpp_f64<DPP_WAVE_SHR1>(rsi);
    if (lane == 0) prsi = rsi_carry;
    rsi_carry = readlane_f64(rsi, WAVE - 1);
    asm volatile("" : "+v"(rsi_carry));
    f[BQ_MR_V_RSI] = rsi;
    f[BQ_MR_V_PREVIOUS_RSI] = prsi;
    f[BQ_MR_V_TREND] = y[3] != 0.0 ? (y[2] - y[3]) / fabs(y[3]) : 0.0;
    f[BQ_MR_V_VOLUME_MA] = window_mean(v, K->p.volume_ma_window, t0, pv_prev, bv_prev);
    f[BQ_MR_V_ATR_MA] = window_mean(a, K->p.atr_ma_window, t0, pa_prev, ba_prev);
  };

  MrStep nxt = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) O.no_frame(t0, BQ_MR_NO_FRAME);
      if (FEAT && any && t0 >= e0 && t0 < b0) {   // the features run from first_t on
        double f[BQ_MR_NFEATURES];
        const bool in = t < T;
        feat_step(in ? cp[t] : qnan(), in ? vp[t] : qnan(), in ? ap[t] : qnan(), t0, f);
      }
      continue;
    }
    if (t0 == b0) nxt = load_step(t0);
    const MrStep cur = nxt;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's arithmetic
    const bool valid = t >= from && t < len;
    const Karg<MrArgs> K = kernarg<MrArgs>();
    const auto& P = K->p;

    double f[BQ_MR_NFEATURES];
    if (FEAT) {
      feat_step(cur.c, cur.v, cur.a, t0, f);
    } else {
#pragma unroll
      for (int k = 0; k < BQ_MR_NFEATURES; ++k) f[k] = cur.f[k];
    }
    const double rsi = f[BQ_MR_V_RSI], prsi = f[BQ_MR_V_PREVIOUS_RSI], vma = f[BQ_MR_V_VOLUME_MA],
                 ama = f[BQ_MR_V_ATR_MA], trend = f[BQ_MR_V_TREND];

    // :252-257
    const bool ready = is_finite(rsi) && is_finite(prsi) && is_finite(vma) && is_finite(cur.a) && is_finite(ama) &&
                       is_finite(trend);
    // :126-147 (compares in the method's direction: a NaN fails)
    const bool spike = cur.a >= P.atr_spike_max * ama;
    const bool lowvol = cur.v < P.volume_ratio_min * vma;
    const double range = cur.h - cur.l;
    const bool badrange = range <= 0.0;
    const double wick = (cur.h - py_max(cur.o, cur.c)) / range;
    const bool setup = rsi >= P.rsi_short_min && rsi < prsi && cur.c >= cur.bb && cur.c < cur.o &&
                       wick >= P.min_wick_ratio;

    // the context and the symbol's snapshot entry at the candle's message
    double cx[5];
    const bool cok = ctx_load(K, ctx_index(K, t, T), cx);
    const double stress = cx[0], longr = cx[1], shortr = cx[2], btc = cx[3], btcret = cx[4];
    bool sok = false;
    double satr = 0.0, strend = 0.0;
    int sreg = BQ_MR_NONE, strans = BQ_MR_NONE;
    if (K->sym_ok) {   // wave-uniform
      const int64_t si = sym_index(K, s, t, T);
      sok = K->sym_ok[si] != 0;
      satr = K->sym_atr[si];
      strend = K->sym_trend[si];
      sreg = K->sym_regime[si];
      strans = K->sym_transition[si];
    }

    int st = BQ_MR_EMIT;
    if (!valid) st = BQ_MR_NO_FRAME;
    else if (!ready) st = BQ_MR_NOT_READY;
    else if (spike) st = BQ_MR_ATR_SPIKE;
    else if (lowvol) st = BQ_MR_LOW_VOLUME;
    else if (badrange) st = BQ_MR_BAD_RANGE;
    else if (!setup) st = BQ_MR_NO_SETUP;
    else if (trend > P.max_trend_score) st = BQ_MR_TREND_TOO_HIGH;                       // :275
    else if (!cok) st = BQ_MR_NO_CONTEXT;                                                // :177
    else if (stress >= P.max_market_stress) st = BQ_MR_STRESS;                           // :179
    else if (sok && satr > P.max_symbol_atr_pct) st = BQ_MR_SYMBOL_ATR;                  // :182
    else if (longr > shortr + P.max_gap) st = BQ_MR_LONG_EDGE;                           // :200-204
    else if (btc > 0.15 && btcret > 0.0) st = BQ_MR_BTC_UP;                              // :205
    else if (sok && strans == BQ_MR_TRANSITION_BREAKOUT_UP) st = BQ_MR_BREAKOUT_UP;      // :208
    else if (sok && sreg == BQ_MR_REGIME_TREND_UP && strend > 0.0) st = BQ_MR_SYMBOL_TREND_UP;   // :210

    // :163-167, :157-161 (unrounded)
    const double pct = ((P.atr_stop_mult * cur.a) / cur.c) * 100.0;
    const double sl = cur.c <= 0.0 ? 0.0 : py_min(py_max(pct, 0.0), 101.0);
    const double score = 1.0 + py_max(0.0, (rsi - P.rsi_short_min) / (100.0 - P.rsi_short_min));
    // :291-300: the entry equals open_time[t] only while no earlier candle of the call has emitted
    const bool pass = st == BQ_MR_EMIT;
    const bool wide = sl > P.max_entry_stop_loss_pct;
    const bool same = pass && has0 && cur.ot == last0;
    const uint64_t EB = __ballot(pass && !same && !wide);
    const uint64_t before = lane ? ~0ull >> (WAVE - lane) : 0ull;
    if (same && !emitted && !(EB & before)) st = BQ_MR_ALREADY_EMITTED;
    else if (pass && wide) st = BQ_MR_STOP_TOO_WIDE;
    const uint64_t EM = __ballot(st == BQ_MR_EMIT);
    if (EM) {   // _mark_emitted: the step's last emit
      last_emit = readlane_i64(cur.ot, 63 - __builtin_clzll(EM));
      emitted = true;
    }

    if (t < T) {
      O.st[t0] = (uint8_t)st;
      const bool stop = st == BQ_MR_EMIT || st == BQ_MR_STOP_TOO_WIDE;
#pragma unroll
      for (int k = 0; k < BQ_MR_NFEATURES; ++k)
        if (O.has(k)) O.val[k][t0] = valid ? f[k] : qnan();
      if (O.has(BQ_MR_V_STOP_LOSS)) O.val[BQ_MR_V_STOP_LOSS][t0] = stop ? sl : qnan();
      if (O.has(BQ_MR_V_SCORE)) O.val[BQ_MR_V_SCORE][t0] = st == BQ_MR_EMIT ? score : qnan();
    }
  }
  if (A.st_has && emitted && lane == 0) {
    A.st_has[s] = 1;
    A.st_last[s] = last_emit;
  }
}

}  // namespace bq

extern "C" void bq_mean_reversion_default_params(bq_mean_reversion_params* p) {
  if (!p) return;
  // MeanReversionFade's class attributes (mean_reversion_fade.py:52-73)
  p->rsi_window = 14;
  p->volume_ma_window = 20;
  p->atr_ma_window = 20;
  p->ema_fast = 20;
  p->ema_slow = 50;
  p->reserved = 0;
  p->rsi_short_min = 76.0;
  p->volume_ratio_min = 0.8;
  p->atr_spike_max = 2.2;
  p->atr_stop_mult = 2.0;
  p->max_entry_stop_loss_pct = 1.5;
  p->max_trend_score = 0.005;
  p->max_market_stress = 0.25;
  p->max_gap = 0.02;
  p->max_symbol_atr_pct = 0.03;
  p->min_wick_ratio = 0.0;
}

extern "C" int bq_mean_reversion_replay(const double* open, const double* high, const double* low,
                                        const double* close, const double* volume, int64_t ld_px, const double* atr,
                                        int64_t ld_atr, const double* bb_upper, int64_t ld_bb,
                                        const int64_t* open_time, int64_t ld_ot, const double* const* features,
                                        int64_t ld_ft, const double* ctx, int64_t ld_ctx, const uint8_t* ctx_ok,
                                        int64_t ctx_T, const uint8_t* sym_ok, const double* sym_atr_pct,
                                        const double* sym_trend_score, const uint8_t* sym_regime,
                                        const uint8_t* sym_transition, int64_t ld_sym, const int64_t* lens,
                                        const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                                        const bq_mean_reversion_params* params, uint8_t* st_has, int64_t* st_last,
                                        uint8_t* status, double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!open || !high || !low || !close || !volume || !atr || !bb_upper || !open_time || !ctx || !status || S < 0 ||
      T < 0 || ld_px < T || ld_atr < T || ld_bb < T || ld_ot < T || ld_out < T || (features && ld_ft < T) ||
      (ld_sym != 0 && ld_sym < T) || (ctx_T != 1 && ctx_T != T) || ld_ctx < ctx_T || ld_ctx > 0x1fffffff ||
      T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  if ((st_has != nullptr) != (st_last != nullptr)) return BQ_EINVAL;
  if (sym_ok && (!sym_atr_pct || !sym_trend_score || !sym_regime || !sym_transition)) return BQ_EINVAL;
  if (features)
    for (int k = 0; k < BQ_MR_NFEATURES; ++k)
      if (!features[k]) return BQ_EINVAL;
  MrArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_mean_reversion_default_params(&A.p);
  const bq_mean_reversion_params& p = A.p;
  if (!all_finite({p.rsi_short_min, p.volume_ratio_min, p.atr_spike_max, p.atr_stop_mult, p.max_entry_stop_loss_pct,
                   p.max_trend_score, p.max_market_stress, p.max_gap, p.max_symbol_atr_pct, p.min_wick_ratio}))
    return BQ_EINVAL;
  if (p.rsi_window < 1 || p.ema_fast < 1 || p.ema_slow < 1 || p.volume_ma_window < 1 ||
      p.volume_ma_window > BQ_MR_MAX_WINDOW || p.atr_ma_window < 1 || p.atr_ma_window > BQ_MR_MAX_WINDOW ||
      p.rsi_short_min == 100.0)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.open = open;
  A.high = high;
  A.low = low;
  A.close = close;
  A.volume = volume;
  A.atr = atr;
  A.bb = bb_upper;
  A.ot = open_time;
  for (int k = 0; k < BQ_MR_NFEATURES; ++k) A.feat[k] = features ? features[k] : nullptr;
  A.ctx = ctx;
  A.ctx_ok = ctx_ok;
  A.sym_ok = sym_ok;
  A.sym_atr = sym_atr_pct;
  A.sym_trend = sym_trend_score;
  A.sym_regime = sym_regime;
  A.sym_transition = sym_transition;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_px = ld_px;
  A.ld_atr = ld_atr;
  A.ld_bb = ld_bb;
  A.ld_ot = ld_ot;
  A.ld_ft = ld_ft;
  A.ld_sym = ld_sym;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.ctx_T = (int)ctx_T;
  A.ld_ctx = (int)ld_ctx;
  ewm_consts(A.ew[0], ewm_alpha_wilder((double)p.rsi_window));   // ewm(alpha=1 / RSI_WINDOW) (:94-99)
  ewm_consts(A.ew[1], ewm_alpha_span((double)p.ema_fast));
  ewm_consts(A.ew[2], ewm_alpha_span((double)p.ema_slow));
  A.st_has = st_has;
  A.st_last = st_last;
  A.status = status;
  replay_values(A.val, A.omask, values);
  const dim3 grid((unsigned)blocks), block(RP_NT);
  hipStream_t st = (hipStream_t)stream;
  if (features) hipLaunchKernelGGL((mean_reversion_kernel<false>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((mean_reversion_kernel<true>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
