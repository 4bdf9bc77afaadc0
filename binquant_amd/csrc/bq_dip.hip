// BuyTheDip.signal() replayed over a [S][T] panel of 15m frames (gfx950;
// strategies/coinrule/buy_the_dip.py:127-243): the frame and null gate, the
// start time, the 6 h reference candle found by time (_find_reference_price,
// :49-57), the change band, _allows_entry and the reclaim of the prior close
// and EMA20. Column t of row s = the method on the message whose frame is
// df.iloc[first_t[s]:t + 1]; the method keeps no state, so a column does not
// depend on the messages before it (the rule table: include/binquant_amd.h).
//
// buy_the_dip_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. the null gate covers the whole frame: "a NaN close was seen" is
//      wave-uniform and carried from step to step, the step's own NaN ballot
//      masked to the lanes at or before the candle. The steps between
//      first_t's and from_t's load close alone (the flag, and the EMA's
//      carry); a row stops reading once the flag is set: every later candle is
//      NOT_READY.
//   2. the reference search: target = close_time[t] - lookback_ms. A probe
//      u0 = t - lookback_ms / dt clamped to [first_t, t - 1] is loaded one step
//      ahead, with the step's columns (close_time[u0], close_time[u0 + 1],
//      close[u0]); dt is the candle spacing the lane saw a step earlier, the
//      quotient is formed in fp64: u0 is only a guess. The lanes that passed
//      the gates above the search accept it when close_time[u0] <= target <
//      close_time[u0 + 1] (exact), and otherwise binary-search [first_t, t],
//      whose ends are known to bracket the target. Both give the largest u
//      with close_time[u] <= target for any ascending row, the reverse scan's
//      answer. On a gap-free grid lane i probes candle t0 + i - 24: the wave
//      reads two runs of close_time and one of close that it streamed three
//      lines ago (L2), and no step waits for a load issued within it.
//   3. ema20, when not given: close.ewm(span, adjust=False, min_periods=1)
//      through bq_replay.h's ewm_step (one series seeded at first_t).
//   16 B in (close, close_time; 24 B with ema20 given) and 1 + 3 x 8 B out per
//   candle, the regime codes 1 B each; the probe re-reads 24 B per lane from
//   L2; no LDS, no atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3; <EMA>): in-pass EMA 92 VGPRs,
//   72 SGPRs, 5 waves / SIMD; ema20 given 75 / 62 / 6. No spills, scratch 0,
//   LDS 0 in both.
//
// Domain: close_time strictly ascending within [first_t, lens).
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// the scanned series: ewm(ema_span) of close, seeded at first_t
struct DipSeries {
  static constexpr int NE = 1, NK = 1, SWITCH = 0;
  static constexpr int set(int) { return 0; }
  static constexpr int seed(int) { return 0; }
  static constexpr bool min_periods(int) { return false; }
};

struct DipArgs {
  const double *close, *ema;
  const int64_t* ct;
  const int8_t *mkt, *micro;
  const int64_t *lens, *first, *from;
  int64_t ld_px, ld_ct, ld_e, ld_sym, ld_out, S;
  int T, ctx_T, omask;
  bq_buy_the_dip_params p;
  Ewm ew[1];
  uint8_t* status;
  double* val[BQ_DIP_NVALUES];
};

struct DipStep {
  double c, cp, e;   // close[t], close[t - 1], ema20[t] (given)
  int64_t ct;        // close_time[t]
  int mk, mr;        // the candle's market regime, the symbol's micro regime (negative: None)
};

// the search's first probe: candle u (-1: none), close_time[u], close_time[u + 1], close[u]
struct DipProbe {
  int u;
  int64_t c0, c1;
  double ref;
};

template <bool EMA>
__global__ __launch_bounds__(RP_NT) void buy_the_dip_kernel(const DipArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const double* __restrict__ cl = A.close + s * A.ld_px;
  const double* __restrict__ em = EMA ? nullptr : A.ema + s * A.ld_e;
  const int64_t* __restrict__ ctp = A.ct + s * A.ld_ct;
  // omask bit k: a BQ_DIP_V_*
  ReplayOut<DipArgs, BQ_DIP_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_DIP_NVALUES; ++k) O.set(k, A.val[k]);

  // one step's columns, candle tb + lane (NaN / 0 past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    DipStep x;
    x.c = in ? cl[u] : qnan();
    x.cp = in && u > 0 ? cl[u - 1] : qnan();
    x.e = EMA ? 0.0 : (in ? em[u] : qnan());
    x.ct = in ? ctp[u] : 0;
    // :170 the regimes of the candle's message
    const Karg<DipArgs> K = kernarg<DipArgs>();
    const int8_t* mktp = K->mkt;
    const int8_t* micp = K->micro;
    x.mk = mktp ? mktp[ctx_index(K, u, T)] : -1;
    x.mr = micp ? micp[sym_index(K, s, u, T)] : -1;
    return x;
  };
  // the spacing of a step's candles as each lane sees it: close_time[t] - close_time[t - 1] (lane 0: lane 1's)
  auto spacing = [&](int64_t ct) {
    const unsigned lo = (unsigned)dpp_i32<DPP_WAVE_SHR1>((int)(ct & 0xffffffffll));
    const int hi = dpp_i32<DPP_WAVE_SHR1>((int)(ct >> 32));
    const int64_t d = ct - (((int64_t)hi << 32) | (int64_t)lo);
    return lane ? d : readlane_i64(d, 1);
  };
  // The probe of step tb, loaded with the step's columns on every lane that has a prior candle in its frame:
  // u0 = t - lookback_ms / dt clamped to [first, t - 1], dt the spacing the lane saw one step earlier (the step
  // itself at the first one). The quotient is formed in fp64: u0 is a guess, the step tests it exactly.
  auto probe = [&](int64_t dt, int tb) {
    const int u = tb + lane;
    DipProbe q = {-1, 0, 0, qnan()};
    if (u > first && u < len && dt > 0) {
      const double back = (double)kernarg<DipArgs>()->p.lookback_ms / (double)dt;
      int u0 = back < (double)(u - first) ? u - (int)back : first;
      u0 = u0 > u - 1 ? u - 1 : u0;
      q.u = u0;
      q.c0 = ctp[u0];
      q.c1 = ctp[u0 + 1];
      q.ref = cl[u0];
    }
    return q;
  };

  const int b0 = R.b0(), e0 = R.e0();
  const bool any = R.any();
  bool nanseen = false;   // a NaN close in [first_t, the step's first candle): wave-uniform
  const int64_t ct_first = any ? ctp[first] : 0;   // the frame's oldest close_time: is there a reference at all

  // ---- the in-pass ewm series: candles t0 .. t0 + 63 into y (every lane executes it)
  EwmState<DipSeries::NE, DipSeries::NK> ES;
  ewm_init<DipSeries>(ES, A.ew, lane, EMA);
  auto ema_step = [&](double c, int t0) {
    const double xs[1] = {win_val(c)};   // ewm: +-inf is missing
    double y[1];
    ewm_step<DipSeries>(ES, kernarg<DipArgs>()->ew, xs, t0, lane, first, len, 0, y);
    return y[0];
  };

  // the next step's columns and probe are loaded before this step's arithmetic: a step waits only for loads
  // issued a step ago (the memory counter retires loads in order)
  DipStep cur = {};
  DipProbe pc = {-1, 0, 0, 0.0};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) O.no_frame(t0, BQ_DIP_NO_FRAME);
      if (any && t0 >= e0 && t0 < b0 && !nanseen) {   // the frame runs from first_t on: close alone
        const double c = t < T ? cl[t] : qnan();
        nanseen = __ballot(t >= first && c != c) != 0;
        if (EMA && !nanseen) ema_step(c, t0);
      }
      continue;
    }
    const bool valid = t >= from && t < len;
    if (nanseen) {   // :139 isnull().any().any(): the rest of the row
      if (t < T) {
        O.st[t0] = valid ? BQ_DIP_NOT_READY : BQ_DIP_NO_FRAME;
#pragma unroll
        for (int k = 0; k < BQ_DIP_NVALUES; ++k)
          if (O.has(k)) O.val[k][t0] = qnan();
      }
      continue;
    }
    if (t0 == b0) {
      cur = load_step(t0);
      pc = probe(spacing(cur.ct), t0);
    }
    DipStep nxt = cur;
    DipProbe pn = pc;
    if (t0 + WAVE < len) {   // in flight during this step's arithmetic
      nxt = load_step(t0 + WAVE);
      pn = probe(spacing(cur.ct), t0 + WAVE);
    }
    const Karg<DipArgs> K = kernarg<DipArgs>();
    const auto& P = K->p;

    // :137-140 the frame and null gate
    const uint64_t NB = __ballot(t >= first && t < len && cur.c != cur.c);
    const bool null = (NB & (~0ull >> (WAVE - 1 - lane))) != 0;
    const bool ready = t + 1 - first >= P.lookback_candles && !null;
    double ema = cur.e;
    if (EMA) ema = ema_step(cur.c, t0);
    nanseen = NB != 0;
    // :147-149
    const bool started = cur.ct >= P.start_time_ms;

    // :152-156 the newest candle of the frame at least lookback_ms older than the message's
    bool found = false;
    double refp = qnan(), change = qnan();
    if (valid && ready && started) {   // t - 1 >= first: lookback_candles >= 2
      const int64_t target = cur.ct - P.lookback_ms;
      if (ct_first <= target) {
        refp = pc.ref;
        if (!(pc.u >= 0 && pc.c0 <= target && pc.c1 > target)) {   // close_time[first] <= target < close_time[t]
          int lo = first, hi = t;
          while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (ctp[mid] <= target) lo = mid;
            else hi = mid;
          }
          refp = cl[lo];
        }
        found = true;
        change = safe_pct(cur.c, refp) * 100.0;   // :158
      }
    }
    // :170 _allows_entry: a trending market, or a trending symbol (negative codes: None)
    const bool blocked = cur.mk == BQ_DIP_REGIME_TREND_UP || cur.mk == BQ_DIP_REGIME_TREND_DOWN ||
                         cur.mr == BQ_DIP_REGIME_TREND_UP || cur.mr == BQ_DIP_REGIME_TREND_DOWN;

    int st = BQ_DIP_EMIT;
    if (!valid) st = BQ_DIP_NO_FRAME;
    else if (!ready) st = BQ_DIP_NOT_READY;
    else if (!started) st = BQ_DIP_BEFORE_START;
    else if (!found) st = BQ_DIP_NO_REFERENCE;
    else if (change > P.max_change_pct || change <= P.min_change_pct) st = BQ_DIP_OUT_OF_BAND;   // :159, a NaN goes on
    else if (blocked) st = BQ_DIP_REGIME_BLOCKED;
    else if (!(cur.c > cur.cp && cur.c > ema)) st = BQ_DIP_NOT_RECLAIMED;   // :59-61

    if (t < T) {
      O.st[t0] = (uint8_t)st;
      const bool searched = st == BQ_DIP_EMIT || st >= BQ_DIP_OUT_OF_BAND;
      const bool reclaim = st == BQ_DIP_EMIT || st == BQ_DIP_NOT_RECLAIMED;
      if (O.has(BQ_DIP_V_REFERENCE)) O.val[BQ_DIP_V_REFERENCE][t0] = searched ? refp : qnan();
      if (O.has(BQ_DIP_V_CHANGE)) O.val[BQ_DIP_V_CHANGE][t0] = searched ? change : qnan();
      if (O.has(BQ_DIP_V_EMA)) O.val[BQ_DIP_V_EMA][t0] = reclaim ? ema : qnan();
    }
    cur = nxt;
    pc = pn;
  }
}

}  // namespace bq

extern "C" void bq_buy_the_dip_default_params(bq_buy_the_dip_params* p) {
  if (!p) return;
  // BuyTheDip's class attributes (:34-36) and signal()'s constants (:67, :159)
  p->lookback_candles = 24;
  p->ema_span = 20;
  p->lookback_ms = 6 * (int64_t)3600000;
  p->start_time_ms = 1776036060000;   // datetime(2026, 4, 12, 23, 21, tzinfo=UTC)
  p->min_change_pct = -5.0;
  p->max_change_pct = -2.0;
}

extern "C" int bq_buy_the_dip_replay(const double* close, int64_t ld_px, const int64_t* close_time, int64_t ld_ct,
                                     const double* ema20, int64_t ld_e, const int8_t* market_regime,
                                     int64_t regime_T, const int8_t* micro_regime, int64_t ld_m,
                                     const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S,
                                     int64_t T, const bq_buy_the_dip_params* params, uint8_t* status,
                                     double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!close || !close_time || !status || S < 0 || T < 0 || ld_px < T || ld_ct < T || ld_out < T ||
      (ema20 && ld_e < T) || (market_regime && regime_T != 1 && regime_T != T) ||
      (micro_regime && ld_m != 0 && ld_m < T) || T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  DipArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_buy_the_dip_default_params(&A.p);
  const bq_buy_the_dip_params& p = A.p;
  if (!all_finite({p.min_change_pct, p.max_change_pct})) return BQ_EINVAL;
  if (!(p.min_change_pct < p.max_change_pct) || p.lookback_candles < 2 || p.lookback_ms <= 0 || p.ema_span < 1)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.close = close;
  A.ct = close_time;
  A.ema = ema20;
  A.mkt = market_regime;
  A.micro = micro_regime;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_px = ld_px;
  A.ld_ct = ld_ct;
  A.ld_e = ld_e;
  A.ld_sym = micro_regime ? ld_m : 0;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.ctx_T = market_regime ? (int)regime_T : 1;
  ewm_consts(A.ew[0], ewm_alpha_span((double)p.ema_span));   // close.ewm(span=20, adjust=False, min_periods=1) (:65-70)
  A.status = status;
  replay_values(A.val, A.omask, values);
  const dim3 grid((unsigned)blocks), block(RP_NT);
  hipStream_t st = (hipStream_t)stream;
  if (ema20) hipLaunchKernelGGL((buy_the_dip_kernel<false>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((buy_the_dip_kernel<true>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
