// PriceTracker.signal() replayed over a [S][T] panel of 5m frames (gfx950;
// strategies/coinrule/price_tracker.py:165-324): the frame and null gate, the
// oversold test and local_score, score_signal_candidate_with_context's LONG
// branch with the three rejections taken from it, and the entry cooldown kept
// in strategy_cooldowns. Column t of row s = the method on the message whose
// frame is df.iloc[first_t[s]:t + 1], after the messages of all earlier
// candles of the row (the rule table: include/binquant_amd.h).
//
// price_tracker_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. the gates and both scores are point-wise, in the method's operation
//      order. tail(tail_rows).isnull() looks back across the step edge: the
//      previous step's NaN ballot is carried (the first replayed step forms it
//      with one extra load of the tail_rows - 1 candles before it).
//   2. the cooldown entry (has, last_close_time) is wave-uniform. The walk
//      takes one iteration per EMIT, not per candle: among the remaining bits
//      of P = ballot(passed every gate above the cooldown) the first lane
//      whose close_time lies outside [last, last + cooldown_ms) emits, the P
//      lanes before it are COOLDOWN, last moves to that lane's close_time.
//   3. trend_score, when not given: closes.ewm(span, adjust=False).mean() for
//      both spans through bq_replay.h's ewm_step (two series seeded at first_t,
//      one input); steps between first_t's and from_t's load close only.
//   Up to 9 x 8 B in (the context rows: L2-resident) and 2 + 6 x 8 B out per
//   candle; no LDS, no atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3; <EMA, HLV>): in-pass EMA with
//   high / low / volume 114 VGPRs, 106 SGPRs, 4 waves / SIMD; in-pass EMA
//   without them 100 / 105 / 4; trend_score given 88 / 106 / 5 and 72 / 106 /
//   7. No spills, scratch 0, LDS 0 in all four.
//
// Domain: close_time strictly ascending within [first_t, lens).
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// the scanned series: ewm(span_fast) and ewm(span_slow) of close, seeded at first_t
struct PtSeries {
  static constexpr int NE = 2, NK = 2, SWITCH = 0;
  static constexpr int set(int e) { return e; }
  static constexpr int seed(int) { return 0; }
  static constexpr bool min_periods(int) { return false; }
};

struct PtArgs {
  const double *close, *rsi, *macd, *mfi, *high, *low, *volume, *trend, *rs, *ctx;
  const int64_t* ct;
  const uint8_t* ctx_ok;
  const int64_t *lens, *first, *from;
  int64_t ld_px, ld_ind, ld_ct, ld_tr, ld_rs, ld_out, S;
  int T, ctx_T, ld_ctx, omask;
  bq_price_tracker_params p;
  Ewm ew[2];   // span_fast, span_slow
  uint8_t* st_has;
  int64_t* st_last;
  uint8_t *status, *detail;
  double* val[BQ_PT_NVALUES];
};

struct PtStep {
  double c, rsi, macd, mfi, h, l, v, tr, rs;
  int64_t ct;
};

// shared/utils.py:12-17, as bq_regime.hip states them
__device__ __forceinline__ double pt_clamp(double x, double lo = -1.0, double hi = 1.0) {
  const double m = x < hi ? x : hi;   // min(high, value)
  return m > lo ? m : lo;              // max(low, m)
}
__device__ __forceinline__ double pt_nneg(double x) { return x > 0.0 ? x : 0.0; }   // max(0.0, value)

template <bool EMA, bool HLV>
__global__ __launch_bounds__(RP_NT) void price_tracker_kernel(const PtArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const int TR0 = A.p.tail_rows;
  constexpr bool ema = EMA;   // trend_score NULL: formed in the pass
  const double* __restrict__ cl = A.close + s * A.ld_px;
  // HLV: high / low / volume join the null test (the host passes close for a NULL one of the three)
  const double* hi = HLV ? A.high + s * A.ld_px : nullptr;
  const double* lo = HLV ? A.low + s * A.ld_px : nullptr;
  const double* vo = HLV ? A.volume + s * A.ld_px : nullptr;
  if (HLV) asm volatile("" : "+v"(hi), "+v"(lo), "+v"(vo));   // VGPRs, as the outputs' pointers
  const double* rsi = A.rsi + s * A.ld_ind;
  const double* macd = A.macd + s * A.ld_ind;
  const double* mfi = A.mfi + s * A.ld_ind;
  if (EMA) asm volatile("" : "+v"(rsi), "+v"(macd), "+v"(mfi));   // the series' constants take their SGPRs
  const double* __restrict__ trn = EMA ? nullptr : A.trend + s * A.ld_tr;
  const double* __restrict__ rsr = A.rs + s * (A.ld_rs ? A.ld_rs : 1);
  const int64_t* __restrict__ ctp = A.ct + s * A.ld_ct;
  const double rs_row = A.ld_rs ? 0.0 : rsr[0];
  // omask bit k: a BQ_PT_V_*; bit BQ_PT_NVALUES: detail, a per-lane pointer like the others
  ReplayOut<PtArgs, BQ_PT_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_PT_NVALUES; ++k) O.set(k, A.val[k]);
  uint8_t* dt_out = A.detail + O.orow;
  asm volatile("" : "+v"(dt_out));

  // the row's cooldown entry: wave-uniform from here on
  bool has = A.st_has && A.st_has[s] != 0;
  int64_t last = has ? A.st_last[s] : 0;

  // a NaN among the six columns of a candle (pandas isnull: +-inf is a value)
  auto null_of = [&](const PtStep& x) {
    return x.c != x.c || x.rsi != x.rsi || x.macd != x.macd || x.h != x.h || x.l != x.l || x.v != x.v;
  };
  // one step's columns, candle tb + lane (NaN / 0 past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u >= 0 && u < T;
    PtStep x;
    x.c = in ? cl[u] : qnan();
    x.rsi = in ? rsi[u] : qnan();
    x.macd = in ? macd[u] : qnan();
    x.mfi = in ? mfi[u] : qnan();
    x.h = HLV ? (in ? hi[u] : qnan()) : 0.0;
    x.l = HLV ? (in ? lo[u] : qnan()) : 0.0;
    x.v = HLV ? (in ? vo[u] : qnan()) : 0.0;
    x.tr = trn ? (in ? trn[u] : qnan()) : 0.0;
    x.rs = A.ld_rs ? (in ? rsr[u] : qnan()) : rs_row;
    x.ct = in ? ctp[u] : 0;
    return x;
  };

  const int b0 = R.b0(), e0 = R.e0();
  const bool any = R.any();

  // the NaN ballot of the step before b0: only its last TR - 1 candles matter
  uint64_t PB = 0;
  if (any && b0 > first && TR0 > 1) {
    const int u = b0 - 1 - lane;   // lane 0 is the newest
    const bool in = lane < TR0 - 1 && u >= first;
    bool bad = false;
    if (in) {
      bad = cl[u] != cl[u] || rsi[u] != rsi[u] || macd[u] != macd[u];
      if (HLV) bad = bad || hi[u] != hi[u] || lo[u] != lo[u] || vo[u] != vo[u];
    }
    PB = __builtin_bitreverse64(__ballot(bad));   // candle b0 - 1 - j: bit 63 - j
  }

  // ---- the in-pass ewm series: candles t0 .. t0 + 63 of both into y (every lane executes it)
  EwmState<PtSeries::NE, PtSeries::NK> ES;
  ewm_init<PtSeries>(ES, A.ew, lane, ema);
  auto ema_step = [&](double c, int t0, double (&y)[2]) {
    const double x = win_val(c);   // ewm: +-inf is missing
    const double xs[2] = {x, x};
    ewm_step<PtSeries>(ES, kernarg<PtArgs>()->ew, xs, t0, lane, first, len, 0, y);
  };

  PtStep nxt = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) {
        O.no_frame(t0, BQ_PT_NO_FRAME);
        if (O.has(BQ_PT_NVALUES)) dt_out[t0] = 0;
      }
      if (ema && any && t0 >= e0 && t0 < b0) {   // the series run from first_t on: close alone
        double y[2];
        ema_step(t < T ? cl[t] : qnan(), t0, y);
      }
      continue;
    }
    if (t0 == b0) nxt = load_step(t0);
    const PtStep cur = nxt;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's walk
    const bool valid = t >= from && t < len;
    const Karg<PtArgs> K = kernarg<PtArgs>();
    const auto& P = K->p;
    const int TR = P.tail_rows;
    const int64_t cd = P.cooldown_ms;

    // :174-181 the frame and null gate
    const uint64_t NB = __ballot(t >= first && t < len && null_of(cur));
    const bool tailbad = window_hit(NB, PB, TR, lane);
    PB = NB;
    const bool ready = t + 1 - first >= P.min_history && !tailbad;
    // :194 (compares in the method's direction: a NaN fails)
    const bool setup = cur.rsi < P.rsi_max && cur.macd < P.macd_max && cur.mfi < P.mfi_max;
    // :198-203
    const double local = ((1.0 + pt_nneg((P.rsi_max - cur.rsi) / P.rsi_max) * P.w_rsi) +
                          pt_nneg((P.mfi_max - cur.mfi) / P.mfi_max) * P.w_mfi) +
                         py_min(fabs(cur.macd) * P.macd_scale, 1.0) * P.w_macd;
    // :204-210
    double trend = cur.tr;
    if (ema) {
      double y[2];
      ema_step(cur.c, t0, y);
      trend = y[1] != 0.0 ? (y[0] - y[1]) / fabs(y[1]) : 0.0;
    }
    // the context of the candle's message
    double cx[4];
    const bool cok = ctx_load(K, ctx_index(K, t, T), cx);
    const double conf = cx[0], tail_l = cx[1], btc = cx[2], stress = cx[3];
    // RuleBasedMarketContextModel.evaluate, LONG (context_scoring.py:22-85)
    double conf_s = 0.0, fol = 0.0, adv = 0.0, sup = 0.0;
    if (cok && !(conf <= 0.0)) {
      const double r = cur.rs;
      const double btc_al = pt_clamp(btc);
      const double cross = pt_clamp(0.6 * r + 0.4 * trend);
      const double over = pt_clamp(0.6 * pt_nneg(r) + 0.4 * pt_nneg(trend), 0.0, 1.0);
      const double dstress = -stress;
      sup = pt_clamp(0.35 * tail_l + 0.25 * btc_al + 0.25 * cross + 0.15 * dstress);
      fol = pt_clamp(0.45 * tail_l + 0.3 * btc_al + 0.25 * cross);
      adv = pt_clamp(0.55 * stress + 0.25 * pt_nneg(-sup) + 0.2 * (1.0 - over), 0.0, 1.0);
      if (tail_l < 0.0 && over > 0.0) {
        sup = pt_clamp(sup + 0.2 * over);
        fol = pt_clamp(fol + 0.15 * over);
      }
      conf_s = conf;
    }
    // SignalContextScorer.adjust_score (signal_context_scorer.py:20-29)
    const double adj = local + conf_s * P.context_weight * (fol + (P.support_weight * sup) - (P.risk_weight * adv));
    // :236-242
    const int rej = (fol < P.min_followthrough ? BQ_PT_D_FOLLOWTHROUGH : 0) | (adv > P.max_risk ? BQ_PT_D_RISK : 0) |
                    (conf_s < P.min_confidence ? BQ_PT_D_CONFIDENCE : 0);
    int st = BQ_PT_EMIT, dt = 0;
    if (!valid) st = BQ_PT_NO_FRAME;
    else if (!ready) st = BQ_PT_NOT_READY;
    else if (!setup) st = BQ_PT_NO_SETUP;
    else if (!cok) st = BQ_PT_NO_CONTEXT;
    else if (rej) {
      st = BQ_PT_CONTEXT_REJECTED;
      dt = rej;
    }

    // :244-251 the cooldown: one iteration per EMIT
    uint64_t rest = __ballot(st == BQ_PT_EMIT);
    if (cd > 0) {
      while (rest) {
        int i;
        if (!has) {
          i = __builtin_ctzll(rest);
        } else {
          const int64_t el = cur.ct - last;   // :92-93
          const uint64_t F = __ballot(!(el >= 0 && el < cd)) & rest;
          if (!F) {   // the window covers the step's remaining candidates
            if ((rest >> lane) & 1) st = BQ_PT_COOLDOWN;
            break;
          }
          i = __builtin_ctzll(F);
        }
        if (((rest >> lane) & 1) && lane < i) st = BQ_PT_COOLDOWN;
        last = readlane_i64(cur.ct, i);   // _mark_entry_cooldown
        has = true;
        rest = i == WAVE - 1 ? 0 : rest & (~0ull << (i + 1));
      }
    }

    if (t < T) {
      O.st[t0] = (uint8_t)st;
      if (O.has(BQ_PT_NVALUES)) dt_out[t0] = (uint8_t)dt;
      const bool reached = st == BQ_PT_EMIT || st >= BQ_PT_NO_CONTEXT;
      if (O.has(BQ_PT_V_LOCAL)) O.val[BQ_PT_V_LOCAL][t0] = reached ? local : qnan();
      if (O.has(BQ_PT_V_TREND)) O.val[BQ_PT_V_TREND][t0] = reached ? trend : qnan();
      if (O.has(BQ_PT_V_FOLLOWTHROUGH)) O.val[BQ_PT_V_FOLLOWTHROUGH][t0] = reached ? fol : qnan();
      if (O.has(BQ_PT_V_RISK)) O.val[BQ_PT_V_RISK][t0] = reached ? adv : qnan();
      if (O.has(BQ_PT_V_SUPPORT)) O.val[BQ_PT_V_SUPPORT][t0] = reached ? sup : qnan();
      if (O.has(BQ_PT_V_ADJUSTED)) O.val[BQ_PT_V_ADJUSTED][t0] = reached ? adj : qnan();
    }
  }
  if (A.st_has && lane == 0) {
    A.st_has[s] = has ? 1 : 0;
    A.st_last[s] = has ? last : 0;
  }
}

}  // namespace bq

extern "C" void bq_price_tracker_default_params(bq_price_tracker_params* p) {
  if (!p) return;
  // PriceTracker.signal()'s constants (:177, :194, :198-205, :237-239) and class attributes (:34-35, :59-63)
  p->min_history = 30;
  p->tail_rows = 5;
  p->span_fast = 9;
  p->span_slow = 21;
  p->rsi_max = 30.0;
  p->macd_max = 0.0;
  p->mfi_max = 20.0;
  p->w_rsi = 0.35;
  p->w_mfi = 0.35;
  p->w_macd = 0.3;
  p->macd_scale = 100.0;
  p->context_weight = 0.35;
  p->risk_weight = 0.35;
  p->support_weight = 0.2;
  p->min_followthrough = -0.2;
  p->max_risk = 0.6;
  p->min_confidence = 0.5;
  p->cooldown_ms = 12 * (int64_t)300000;   // ENTRY_COOLDOWN_BARS x DEFAULT_INTERVAL_MS
}

extern "C" int bq_price_tracker_replay(const double* close, const double* high, const double* low,
                                       const double* volume, int64_t ld_px, const double* rsi, const double* macd,
                                       const double* mfi, int64_t ld_ind, const int64_t* close_time, int64_t ld_ct,
                                       const double* trend_score, int64_t ld_tr, const double* symbol_rs,
                                       int64_t ld_rs, const double* ctx, int64_t ld_ctx, const uint8_t* ctx_ok,
                                       int64_t ctx_T, const int64_t* lens, const int64_t* first_t,
                                       const int64_t* from_t, int64_t S, int64_t T,
                                       const bq_price_tracker_params* params, uint8_t* st_has, int64_t* st_last,
                                       uint8_t* status, uint8_t* detail, double* const* values, int64_t ld_out,
                                       void* stream) {
  using namespace bq;
  if (!close || !rsi || !macd || !mfi || !close_time || !symbol_rs || !ctx || !status || S < 0 || T < 0 ||
      ld_px < T || ld_ind < T || ld_ct < T || ld_out < T || (trend_score && ld_tr < T) || (ld_rs != 0 && ld_rs < T) ||
      (ctx_T != 1 && ctx_T != T) || ld_ctx < ctx_T || ld_ctx > 0x1fffffff || T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  if ((st_has != nullptr) != (st_last != nullptr)) return BQ_EINVAL;
  PtArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_price_tracker_default_params(&A.p);
  const bq_price_tracker_params& p = A.p;
  if (!all_finite({p.rsi_max, p.macd_max, p.mfi_max, p.w_rsi, p.w_mfi, p.w_macd, p.macd_scale, p.context_weight,
                   p.risk_weight, p.support_weight, p.min_followthrough, p.max_risk, p.min_confidence}))
    return BQ_EINVAL;
  if (p.min_history < 1 || p.tail_rows < 1 || p.tail_rows > BQ_PT_MAX_TAIL_ROWS || p.span_fast < 1 ||
      p.span_slow < 1 || p.cooldown_ms < 0 || p.rsi_max == 0.0 || p.mfi_max == 0.0)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.close = close;
  const bool hlv = high || low || volume;   // a NULL one of the three: close stands in (tested anyway)
  A.high = high ? high : close;
  A.low = low ? low : close;
  A.volume = volume ? volume : close;
  A.rsi = rsi;
  A.macd = macd;
  A.mfi = mfi;
  A.ct = close_time;
  A.trend = trend_score;
  A.rs = symbol_rs;
  A.ctx = ctx;
  A.ctx_ok = ctx_ok;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_px = ld_px;
  A.ld_ind = ld_ind;
  A.ld_ct = ld_ct;
  A.ld_tr = ld_tr;
  A.ld_rs = ld_rs;
  A.ld_ctx = (int)ld_ctx;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.ctx_T = (int)ctx_T;
  ewm_consts(A.ew[0], ewm_alpha_span((double)p.span_fast));   // close.ewm(span=9, adjust=False) (:204)
  ewm_consts(A.ew[1], ewm_alpha_span((double)p.span_slow));   // close.ewm(span=21, adjust=False) (:205)
  A.st_has = st_has;
  A.st_last = st_last;
  A.status = status;
  A.detail = detail;
  replay_values(A.val, A.omask, values);
  A.omask |= detail ? 1 << BQ_PT_NVALUES : 0;
  const dim3 grid((unsigned)blocks), block(RP_NT);
  hipStream_t st = (hipStream_t)stream;
  if (trend_score && hlv) hipLaunchKernelGGL((price_tracker_kernel<false, true>), grid, block, 0, st, A);
  else if (trend_score) hipLaunchKernelGGL((price_tracker_kernel<false, false>), grid, block, 0, st, A);
  else if (hlv) hipLaunchKernelGGL((price_tracker_kernel<true, true>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((price_tracker_kernel<true, false>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
