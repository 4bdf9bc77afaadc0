// GradualGainerRetest.signal()'s watchlist state machine replayed over a
// [S][T] panel (gfx950; strategies/gradual_gainer_retest.py:222-308): a leader
// candle opens a watch with a breakout level, the watch expires by wall-clock
// time, a shallow, supported, green reclaim inside it becomes the candidate,
// a risk veto keeps it alive. Column t of row s = the method on the message
// whose frame is df.iloc[first_t[s]:t + 1], after the messages of all earlier
// candles of the row (the semantics table: include/binquant_amd.h).
//
// retest_kernel: the wave-per-row replay mapping (bq_replay.h; from_t is taken
// as given: candles before first_t are SHORT_HISTORY, not skipped).
//   1. each lane forms its candle's state-independent values: frame long
//      enough, leader, green reclaim, risk, the EMA arm of the support test,
//      the t - 1 values (the neighbouring lane; lane 0 takes the previous
//      step's lane 63 from scalar registers) and the maximum of the L highs
//      before it (NaN skipped; the lanes before it and the previous step's
//      high register) — formed only in steps that hold a leader candle.
//   2. the state (active, started_at, level) is wave-uniform. The walk takes
//      one iteration per STATE CHANGE, not per candle: idle, it jumps to the
//      first leader bit of the step's ballot mask and reads that lane's open
//      time and level (readlane); watching, the level-dependent tests of all
//      lanes are formed at once against the uniform level (one multiply each,
//      in the reference's direction: a NaN fails), and the watch ends at the
//      first set bit of ballot(candidate) or of ballot(open_time > expires_at),
//      whichever is earlier. The lanes of the interval in between take their
//      event, detail bits and level from the iteration that covered them.
//   The next step's columns are loaded before this step's walk, so the loads
//   are in flight while the wave walks (0.420 -> 0.378 ms at 12.5k x 2k).
//   Inputs cross HBM once: 50 B in + 10 B out per candle with every column.
//
// Domain: open_time strictly ascending within [first_t, lens): the
// strategy_cooldowns check (:275-282) needs two messages with one open_time
// and is not built.
#include "bq_replay.h"
#include "binquant_amd.h"

namespace bq {

struct RetestArgs {
  const double *open, *high, *low, *close, *ema;
  const int64_t* ts;
  const uint8_t *leader, *risk;
  const int64_t *lens, *first, *from;
  int64_t ld_in, ld_ts, ld_b, ld_out, S;
  int T;
  bq_retest_params p;
  uint8_t* st_active;
  int64_t* st_started;
  double* st_level;
  uint8_t *event, *detail;
  double* level;
};

struct RetestStep {
  double o, h, l, c, e;
  int64_t ot;
  uint8_t lead, risk;
};

__global__ __launch_bounds__(RP_NT) void retest_kernel(const RetestArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const ReplayRow R = replay_row<false>(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const bq_retest_params P = A.p;
  const int L = P.breakout_lookback;
  const double sf = P.support_factor, pf = P.pullback_factor;
  const double* __restrict__ op = A.open + s * A.ld_in;
  const double* __restrict__ hi = A.high + s * A.ld_in;
  const double* __restrict__ lo = A.low + s * A.ld_in;
  const double* __restrict__ cl = A.close + s * A.ld_in;
  const double* __restrict__ em = A.ema + s * A.ld_in;
  const int64_t* __restrict__ ts = A.ts + s * A.ld_ts;
  const uint8_t* __restrict__ ld = A.leader + s * A.ld_b;
  const uint8_t* __restrict__ rk = A.risk ? A.risk + s * A.ld_b : nullptr;
  uint8_t* __restrict__ ev_out = A.event + s * A.ld_out;
  uint8_t* __restrict__ dt_out = A.detail ? A.detail + s * A.ld_out : nullptr;
  double* __restrict__ lv_out = A.level ? A.level + s * A.ld_out : nullptr;

  // the row's state: wave-uniform from here on
  bool active = A.st_active && A.st_active[s] != 0;
  int64_t started = active ? A.st_started[s] : 0;
  double level = active ? A.st_level[s] : qnan();

  const int b0 = R.b0();
  double h_prev_step = qnan();          // lane j: high[t0 - 64 + j]
  double c_h = qnan(), c_l = qnan(), c_c = qnan(), c_e = qnan();   // candle t0 - 1 (uniform)
  // one step's columns, candle tb + lane (NaN / 0 past the row's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    RetestStep x;
    x.o = in ? op[u] : qnan();
    x.h = in ? hi[u] : qnan();
    x.l = in ? lo[u] : qnan();
    x.c = in ? cl[u] : qnan();
    x.e = in ? em[u] : qnan();
    x.ot = in ? ts[u] : 0;
    x.lead = in ? ld[u] : 0;
    x.risk = rk ? (in ? rk[u] : 0) : 1;
    return x;
  };
  RetestStep nxt = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!R.any() || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) {
        ev_out[t] = BQ_RT_NO_FRAME;
        if (dt_out) dt_out[t] = 0;
        if (lv_out) lv_out[t] = qnan();
      }
      continue;
    }
    if (t0 == b0) {
      nxt = load_step(t0);
      if (t0 > 0) {   // what the first step reads of the candles before it
        h_prev_step = hi[t0 - WAVE + lane];
        c_h = hi[t0 - 1];
        c_l = lo[t0 - 1];
        c_c = cl[t0 - 1];
        c_e = em[t0 - 1];
      }
    }
    const RetestStep cur = nxt;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's walk
    const bool in = t < T;
    const double o = cur.o, h = cur.h, l = cur.l, c = cur.c, e = cur.e;
    const int64_t ot = cur.ot;
    const bool lead = cur.lead != 0, risk = cur.risk != 0;
    // candle t - 1
    const double sh = __shfl_up(h, 1), sl = __shfl_up(l, 1), sc = __shfl_up(c, 1), se = __shfl_up(e, 1);
    const double h1 = lane ? sh : c_h, l1 = lane ? sl : c_l, c1 = lane ? sc : c_c, e1 = lane ? se : c_e;
    const bool inframe = t >= from && t < len;
    const bool valid = inframe && t + 1 - first >= P.min_history;   // :228-235
    const bool green = c > o && c > h1;                             // :266-268
    const bool sup_ema = l1 >= e1 * sf;                             // :262
    const uint64_t V = __ballot(valid);
    const uint64_t LD = __ballot(lead) & V;
    // max(high[t-L .. t-1]) skipping NaN (:247-249); the window lies inside the frame (L < min_history)
    double hm = qnan();
    if (LD) {
      for (int k = 1; k <= L; ++k) {
        const int src = lane - k;
        const double a = __shfl(h, src & (WAVE - 1)), b = __shfl(h_prev_step, src & (WAVE - 1));
        const double v = src >= 0 ? a : b;
        hm = (v > hm || hm != hm) ? v : hm;
      }
    }
    int ev = valid ? BQ_RT_IDLE : inframe ? BQ_RT_SHORT_HISTORY : BQ_RT_NO_FRAME;
    int dt = 0;
    double lv = qnan();
    int pos = 0;   // candles before lane `pos` are decided
    while (pos < WAVE) {
      const uint64_t rest = V & (~0ull << pos);
      if (!rest) break;
      if (!active) {
        const uint64_t m = LD & rest;
        if (!m) break;   // idle to the end of the step (:252-253)
        const int i = __builtin_ctzll(m);
        started = readlane_i64(ot, i);   // _set_watchlist (:119-125, :244-251)
        level = readlane_f64(hm, i);
        active = true;
        if (lane == i) {
          ev = BQ_RT_WATCH_SET;
          lv = level;
        }
        pos = i + 1;
      } else {
        const int64_t expires = started + P.watch_ms;
        const bool sup = l1 >= level * sf || sup_ema;   // :260-262
        const bool pul = c1 >= level * pf;              // :263-265
        const bool all3 = sup && pul && green;
        const uint64_t X = __ballot(ot > expires) & rest;    // :239
        const uint64_t C = __ballot(all3 && risk) & rest;    // :269-274
        const int x = X ? __builtin_ctzll(X) : WAVE, k = C ? __builtin_ctzll(C) : WAVE;
        const int end = x < k ? x : k;
        if (valid && lane >= pos && lane <= end && (lane < end || k < x)) {   // the watch is in force
          ev = lane == end ? BQ_RT_CANDIDATE : all3 ? BQ_RT_RISK_BLOCKED : BQ_RT_WATCHING;
          dt = all3 ? 0 : (sup ? 0 : BQ_RT_D_SUPPORT) | (pul ? 0 : BQ_RT_D_PULLBACK) | (green ? 0 : BQ_RT_D_RECLAIM);
          lv = level;
        }
        if (end == WAVE) break;   // still watching at the step's end
        active = false;           // _clear_watchlist: the candidate (:308) or the expiry (:240)
        started = 0;
        level = qnan();
        if (k < x) {
          pos = k + 1;
        } else {
          if (lane == x) dt = BQ_RT_D_EXPIRED;
          pos = x;   // candle x goes on as an idle candle
        }
      }
    }
    if (in) {
      ev_out[t] = (uint8_t)ev;
      if (dt_out) dt_out[t] = (uint8_t)dt;
      if (lv_out) lv_out[t] = lv;
    }
    h_prev_step = h;
    c_h = readlane_f64(h, WAVE - 1);
    c_l = readlane_f64(l, WAVE - 1);
    c_c = readlane_f64(c, WAVE - 1);
    c_e = readlane_f64(e, WAVE - 1);
  }
  if (A.st_active && lane == 0) {
    A.st_active[s] = active ? 1 : 0;
    A.st_started[s] = started;
    A.st_level[s] = level;
  }
}

}  // namespace bq

extern "C" void bq_retest_default_params(bq_retest_params* p) {
  if (!p) return;
  // GradualGainerRetest's class attributes (:78-85)
  p->watch_ms = 8 * (int64_t)3600000;
  p->min_history = 100;
  p->breakout_lookback = 8;
  p->support_factor = 1 - 0.5 / 100;   // 1 - SUPPORT_TOLERANCE_PCT / 100 (:261)
  p->pullback_factor = 1 - 0.04;       // 1 - MAX_PULLBACK_PCT (:264)
}

extern "C" int bq_retest_replay(const double* open, const double* high, const double* low, const double* close,
                                const double* ema, int64_t ld_in, const int64_t* open_time, int64_t ld_ts,
                                const uint8_t* leader, const uint8_t* risk_ok, int64_t ld_b, const int64_t* lens,
                                const int64_t* first_t, const int64_t* from_t, int64_t S, int64_t T,
                                const bq_retest_params* params, uint8_t* st_active, int64_t* st_started,
                                double* st_level, uint8_t* event, uint8_t* detail, double* level, int64_t ld_out,
                                void* stream) {
  using namespace bq;
  if (!open || !high || !low || !close || !ema || !open_time || !leader || !event || S < 0 || T < 0 || ld_in < T ||
      ld_ts < T || ld_b < T || ld_out < T || T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  const int nstate = (st_active != nullptr) + (st_started != nullptr) + (st_level != nullptr);
  if (nstate != 0 && nstate != 3) return BQ_EINVAL;
  RetestArgs A;
  if (params) A.p = *params;
  else bq_retest_default_params(&A.p);
  if (A.p.breakout_lookback < 1 || A.p.breakout_lookback > BQ_RETEST_MAX_LOOKBACK ||
      A.p.breakout_lookback >= A.p.min_history || A.p.watch_ms < 0)
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.open = open;
  A.high = high;
  A.low = low;
  A.close = close;
  A.ema = ema;
  A.ts = open_time;
  A.leader = leader;
  A.risk = risk_ok;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_in = ld_in;
  A.ld_ts = ld_ts;
  A.ld_b = ld_b;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.st_active = st_active;
  A.st_started = st_started;
  A.st_level = st_level;
  A.event = event;
  A.detail = detail;
  A.level = level;
  hipLaunchKernelGGL(retest_kernel, dim3((unsigned)blocks), dim3(RP_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
