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
// mean_reversion_kernel: price_tracker_kernel's mapping (bq_pricetracker.hip) —
// one wave per row, 64 candles per step, every column one coalesced load per
// step, the next step's columns loaded before this step's arithmetic.
//   1. <FEAT = true> forms the five features over the frame starting at
//      first_t; steps between first_t's and from_t's load close / volume / atr
//      only.
//      - _rsi (:88-109): diff() across the step edge (lane 63's close is
//        carried), clip, and the two ewm(alpha = 1 / 14, min_periods = 14,
//        adjust=False) means as affine maps y -> la y + lb x, one DPP wave scan
//        per step and series with the previous step's carry. A flat stretch
//        scans zeros to exactly 0 + 0 -> 50.0; a loss-free rally leaves the
//        loss mean exactly 0 -> 100 g / g. previous_rsi is the lane to the
//        left, or the previous step's lane 63.
//      - _trend_score (:149-155): the same scan for ewm(span = 20 / 50).
//      - a row that meets a NaN or infinite close inside its frame continues
//        from that step with pandas' own recursion for all four series,
//        serially over the step's lanes (wave-uniform state, per-series
//        observation counts for min_periods).
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
#include "bq_device.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

constexpr int MR_NT = 256;            // threads: MR_NT / WAVE rows per workgroup
constexpr int MR_WPB = MR_NT / WAVE;
constexpr int MR_NE = 4;              // scanned series: gain, loss, ema_fast, ema_slow

// one ewm constant set: pandas' alpha / old-weight factor, the affine map
// y -> la y + lb x, apow[j] = la^(2^j)
struct MrEwm {
  double alpha, om, la, lb;
  double apow[7];
};

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
  MrEwm ew[3];   // Wilder (gain and loss), span ema_fast, span ema_slow
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

// Python's max(a, b) / min(a, b): the first argument unless the second wins the compare
__device__ __forceinline__ double mr_pymax(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double mr_pymin(double a, double b) { return b < a ? b : a; }
// math.isfinite
__device__ __forceinline__ bool mr_finite(double x) { return x - x == 0.0; }
// bits [a, b] of a 64-bit ballot, 0 <= a <= b <= 63
__device__ __forceinline__ uint64_t mr_bits(int a, int b) { return (~0ull >> (63 - b)) & (~0ull << a); }

// The thresholds and ewm constants are read from the kernarg segment where a
// step uses them, through a pointer the compiler cannot see through (as
// bq_pricetracker.hip does): as loop invariants they would be held in SGPRs
// beside the row pointers, and spill. They stay in the scalar cache.
typedef const __attribute__((address_space(4))) MrArgs* MrKarg;
__device__ __forceinline__ MrKarg mr_karg() {
  MrKarg k = (MrKarg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

template <bool FEAT>
__global__ __launch_bounds__(MR_NT) void mean_reversion_kernel(const MrArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = (int64_t)blockIdx.x * MR_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const int len = clamp_row(A.lens, s, T, T), first = clamp_row(A.first, s, 0, T), from0 = clamp_row(A.from, s, 0, T);
  const int from = from0 > first ? from0 : first;   // a candle before first_t has an empty frame: no message
  const double* __restrict__ op = A.open + s * A.ld_px;
  const double* __restrict__ hp = A.high + s * A.ld_px;
  const double* __restrict__ lp = A.low + s * A.ld_px;
  const double* __restrict__ cp = A.close + s * A.ld_px;
  const double* __restrict__ vp = A.volume + s * A.ld_px;
  const double* __restrict__ ap = A.atr + s * A.ld_atr;
  const double* __restrict__ bp = A.bb + s * A.ld_bb;
  const int64_t* __restrict__ otp = A.ot + s * A.ld_ot;
  // the outputs as per-lane pointers held in VGPRs (candle `lane` of the row; a step adds t0), their presence as
  // the bits of A.omask
  const int64_t orow = s * A.ld_out + lane;
  uint8_t* st_out = A.status + orow;
  asm volatile("" : "+v"(st_out));
  double* vout[BQ_MR_NVALUES];
#pragma unroll
  for (int k = 0; k < BQ_MR_NVALUES; ++k) {
    vout[k] = A.val[k] + orow;
    asm volatile("" : "+v"(vout[k]));
  }
  auto has_out = [&](int k) { return (mr_karg()->omask >> k) & 1; };

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
        const double* fp = mr_karg()->feat[k] + s * mr_karg()->ld_ft;
        x.f[k] = in ? fp[u] : qnan();
      }
    }
    x.ot = in ? otp[u] : 0;
    return x;
  };

  const int b0 = from & ~(WAVE - 1);       // the first step that holds a replayed candle
  const int e0 = first & ~(WAVE - 1);      // the first step that holds a candle of the frame
  const bool any = from < len;

  // ---- the in-pass features' state
  double lpow[3] = {0.0, 0.0, 0.0}, rpow[3] = {0.0, 0.0, 0.0}, carry[MR_NE] = {0.0, 0.0, 0.0, 0.0};
  double close_carry = qnan(), rsi_carry = qnan();
  bool serial = false;
  double swv[MR_NE] = {qnan(), qnan(), qnan(), qnan()}, sowt[MR_NE] = {1.0, 1.0, 1.0, 1.0};
  int snobs[2] = {0, 0};
  dd pv_prev = {0.0, 0.0}, pa_prev = {0.0, 0.0};   // the previous step's prefixes of volume / atr
  uint64_t bv_prev = 0, ba_prev = 0;               // and its missing-value ballots
  if (FEAT) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      lpow[e] = pow_bits<7>(A.ew[e].apow, lane + 1);
      rpow[e] = pow_bits<5>(A.ew[e].apow, (lane & 15) + 1);
    }
  }

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
    const int w0 = lane - w + 1;
    bool bad = (NB & mr_bits(w0 > 0 ? w0 : 0, lane)) != 0;
    if (w0 < 0) bad = bad || (bprev >> (WAVE + w0)) != 0;
    pprev = P;
    bprev = NB;
    return (t + 1 - first >= w && !bad) ? dd_round(sum) / (double)w : qnan();
  };

  // candles t0 .. t0 + 63: rsi, previous_rsi, volume_ma, atr_ma, trend_score into f (every lane executes it;
  // called once for every step from e0 on, in order)
  auto feat_step = [&](double c, double v, double a, int t0, double (&f)[BQ_MR_NFEATURES]) {
    const int t = t0 + lane;
    const MrKarg K = mr_karg();
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
    if (!serial && __ballot(t >= first && t < len && !(x[2] == x[2]))) {   // wave-uniform: the row turns serial here
      serial = true;
#pragma unroll
      for (int e = 0; e < MR_NE; ++e) {
        // candles first (+ 1 for the differences) .. t0 - 1 were all observations
        const bool seeded = e < 2 ? t0 > first + 1 : t0 > first;
        swv[e] = seeded ? carry[e] : qnan();
        sowt[e] = 1.0;
      }
      snobs[0] = snobs[1] = t0 > first ? t0 - 1 - first : 0;
    }
    if (serial) {   // pandas' recursion over the step, all four series
      const double om[3] = {K->ew[0].om, K->ew[1].om, K->ew[2].om};
      const double alpha[3] = {K->ew[0].alpha, K->ew[1].alpha, K->ew[2].alpha};
      const int i0 = first > t0 ? first - t0 : 0, n = len - t0 < WAVE ? len - t0 : WAVE;
#pragma unroll
      for (int e = 0; e < MR_NE; ++e) y[e] = qnan();
      for (int i = i0; i < n; ++i) {
#pragma unroll
        for (int e = 0; e < MR_NE; ++e) {
          const int k = e < 2 ? 0 : e - 1;
          const double cur = readlane_f64(x[e], i);
          const bool obs = cur == cur;
          double wv = swv[e], owt = sowt[e];
          if (t0 + i == first) {
            wv = cur;
            owt = 1.0;
            if (e < 2) snobs[e] = obs ? 1 : 0;
          } else {
            if (e < 2) snobs[e] += obs ? 1 : 0;
            if (wv == wv) {
              owt *= om[k];
              if (obs) {
                if (wv != cur) {
                  wv = owt * wv + alpha[k] * cur;
                  wv /= owt + alpha[k];
                }
                owt = 1.0;
              }
            } else if (obs) {
              wv = cur;
            }
          }
          swv[e] = wv;
          sowt[e] = owt;
          asm volatile("" : "+v"(swv[e]), "+v"(sowt[e]));
          if (lane == i) y[e] = (e < 2 && snobs[e] < W) ? qnan() : wv;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < MR_NE; ++e) {
        const int k = e < 2 ? 0 : e - 1;
        const int seed = e < 2 ? first + 1 : first;
        const double apw[5] = {K->ew[k].apow[0], K->ew[k].apow[1], K->ew[k].apow[2], K->ew[k].apow[3],
                               K->ew[k].apow[4]};
        // zero before the seed, the seed itself: its lane receives a zero carry
        const double b = t < seed ? 0.0 : (t == seed ? x[e] : K->ew[k].lb * x[e]);
        const double inc = wave_scan_affine_dpp_rp(b, apw, rpow[k], lane);
        y[e] = fma(lpow[k], carry[e], inc);
        carry[e] = readlane_f64(y[e], WAVE - 1);
        asm volatile("" : "+v"(carry[e]));   // the series' uniform state lives in VGPRs, not beside the row pointers
        if (e < 2 && t - first < W) y[e] = qnan();   // min_periods: t - first differences so far
      }
    }
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
      if (t < T) {
        st_out[t0] = BQ_MR_NO_FRAME;
#pragma unroll
        for (int k = 0; k < BQ_MR_NVALUES; ++k)
          if (has_out(k)) vout[k][t0] = qnan();
      }
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
    const MrKarg K = mr_karg();
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
    const bool ready = mr_finite(rsi) && mr_finite(prsi) && mr_finite(vma) && mr_finite(cur.a) && mr_finite(ama) &&
                       mr_finite(trend);
    // :126-147 (compares in the method's direction: a NaN fails)
    const bool spike = cur.a >= P.atr_spike_max * ama;
    const bool lowvol = cur.v < P.volume_ratio_min * vma;
    const double range = cur.h - cur.l;
    const bool badrange = range <= 0.0;
    const double wick = (cur.h - mr_pymax(cur.o, cur.c)) / range;
    const bool setup = rsi >= P.rsi_short_min && rsi < prsi && cur.c >= cur.bb && cur.c < cur.o &&
                       wick >= P.min_wick_ratio;

    // the context and the symbol's snapshot entry at the candle's message
    unsigned ci = K->ctx_T == 1 ? 0u : (unsigned)(t < T ? t : 0);
    asm volatile("" : "+v"(ci));   // vector loads also where the context is one column
    const unsigned ldc = (unsigned)K->ld_ctx;
    const uint8_t* cokp = K->ctx_ok;
    const double* ctxp = K->ctx;
    const bool cok = cokp ? cokp[ci] != 0 : true;
    const double stress = ctxp[ci], longr = ctxp[ldc + ci], shortr = ctxp[2 * ldc + ci], btc = ctxp[3 * ldc + ci],
                 btcret = ctxp[4 * ldc + ci];
    bool sok = false;
    double satr = 0.0, strend = 0.0;
    int sreg = BQ_MR_NONE, strans = BQ_MR_NONE;
    if (K->sym_ok) {   // wave-uniform
      const int64_t lds = K->ld_sym;
      int64_t si = lds ? s * lds + (t < T ? t : 0) : s;
      asm volatile("" : "+v"(si));
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
    const double sl = cur.c <= 0.0 ? 0.0 : mr_pymin(mr_pymax(pct, 0.0), 101.0);
    const double score = 1.0 + mr_pymax(0.0, (rsi - P.rsi_short_min) / (100.0 - P.rsi_short_min));
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
      st_out[t0] = (uint8_t)st;
      const bool stop = st == BQ_MR_EMIT || st == BQ_MR_STOP_TOO_WIDE;
#pragma unroll
      for (int k = 0; k < BQ_MR_NFEATURES; ++k)
        if (has_out(k)) vout[k][t0] = valid ? f[k] : qnan();
      if (has_out(BQ_MR_V_STOP_LOSS)) vout[BQ_MR_V_STOP_LOSS][t0] = stop ? sl : qnan();
      if (has_out(BQ_MR_V_SCORE)) vout[BQ_MR_V_SCORE][t0] = st == BQ_MR_EMIT ? score : qnan();
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

namespace {
void mr_ewm_consts(bq::MrEwm& E, double alpha) {
  E.alpha = alpha;
  E.om = 1.0 - alpha;
  const double den = E.om + E.alpha;
  E.la = E.om / den;
  E.lb = E.alpha / den;
  E.apow[0] = E.la;
  for (int j = 1; j < 7; ++j) E.apow[j] = E.apow[j - 1] * E.apow[j - 1];
}
}  // namespace

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
  const double fin[] = {p.rsi_short_min,   p.volume_ratio_min,  p.atr_spike_max, p.atr_stop_mult,
                        p.max_entry_stop_loss_pct, p.max_trend_score, p.max_market_stress, p.max_gap,
                        p.max_symbol_atr_pct, p.min_wick_ratio};
  for (double v : fin)
    if (!(v - v == 0.0)) return BQ_EINVAL;
  if (p.rsi_window < 1 || p.ema_fast < 1 || p.ema_slow < 1 || p.volume_ma_window < 1 ||
      p.volume_ma_window > BQ_MR_MAX_WINDOW || p.atr_ma_window < 1 || p.atr_ma_window > BQ_MR_MAX_WINDOW ||
      p.rsi_short_min == 100.0)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  const int64_t blocks = (S + MR_WPB - 1) / MR_WPB;
  if (blocks > 0x7fffffff) return BQ_EINVAL;
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
  // pandas keeps com and forms alpha = 1 / (1 + com) from it: com = (1 - alpha) / alpha for ewm(alpha=1 / RSI_WINDOW)
  // (:94-99), com = (span - 1) / 2 for ewm(span=)
  const double wa = 1.0 / (double)p.rsi_window;
  mr_ewm_consts(A.ew[0], 1.0 / (1.0 + (1.0 - wa) / wa));
  mr_ewm_consts(A.ew[1], 1.0 / (1.0 + ((double)p.ema_fast - 1.0) / 2.0));
  mr_ewm_consts(A.ew[2], 1.0 / (1.0 + ((double)p.ema_slow - 1.0) / 2.0));
  A.st_has = st_has;
  A.st_last = st_last;
  A.status = status;
  for (int k = 0; k < BQ_MR_NVALUES; ++k) {
    A.val[k] = values ? values[k] : nullptr;
    A.omask |= A.val[k] ? 1 << k : 0;
  }
  const dim3 grid((unsigned)blocks), block(MR_NT);
  hipStream_t st = (hipStream_t)stream;
  if (features) hipLaunchKernelGGL((mean_reversion_kernel<false>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((mean_reversion_kernel<true>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
