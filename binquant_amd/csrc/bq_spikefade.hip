// FailedSpikeFade.signal()'s pending-spike state machine replayed over a
// [S][T] panel (gfx950; strategies/failed_spike_fade.py:596-695): a qualified
// bullish spike is recorded while the source gates allow it; within
// window_bars candles it is cleared by a high that extends too far beyond the
// spike's, becomes the candidate on a failed new high under the failure market
// gate, or the window runs out. Column t of row s = the method on the message
// whose frame is df.iloc[first_t[s]:t + 1], after the messages of all earlier
// candles of the row (the rule table: include/binquant_amd.h).
//
// spike_fade_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. the state (active, the spike's open_time / high / close, and its
//      position p) is wave-uniform. Inside a replay the kernel knows p: it set
//      it. A carried-in spike is looked up once per row before the first step,
//      backwards from from_t in 64-wide ballots, until the hit, first_t, or an
//      older open time (the domain is ascending): not found -> candle_expired
//      on the first candle.
//   2. the walk takes one iteration per STATE CHANGE, not per candle: idle, it
//      jumps to the first bit of ballot(source_ok & src_market); pending, the
//      tests of all lanes are formed at once against the uniform spike (one
//      multiply, compares in the method's direction: a NaN fails), and the
//      interval ends at the earliest set bit of three ballots — bars >
//      window_bars, the extension, the candidate — the method's order
//      deciding between bits of one candle. Several set / resolve cycles can
//      fall inside one step. A cleared spike consumes its candle.
//   3. post_high = max(high[p+1 .. t]) (NaN skipped) > thr holds iff some
//      high[u] > thr, u in (p, t]; a spike still pending at t saw no such u
//      among the candles replayed since p. So the extension bit of lane t is
//      high[t] > thr alone, and the window's maximum is never formed. Only a
//      carried-in spike has candles in (p, from_t) this launch did not replay:
//      their highs are tested once, with the look-up (at most window_bars of
//      them, one load), and join from_t's bit.
//   24 B + 8 B + 1 B in (the market masks: one shared row, L2-resident) and up
//   to 3 B out per candle; no LDS, no scratch.
//   Resource usage (gfx950 cross-compile, -O3): 38 VGPRs, 105 SGPRs, no spills,
//   scratch 0, LDS 0, 7 waves / SIMD.
//
// Domain: open_time strictly ascending within [first_t, lens), as for the
// retest replay: the spike's position is unique.
#include "bq_replay.h"
#include "binquant_amd.h"

namespace bq {

struct SpikeFadeArgs {
  const double *open, *high, *close;
  const int64_t* ts;
  const uint8_t *source, *src_market, *fail_market;
  const int64_t *lens, *first, *from;
  int64_t ld_in, ld_ts, ld_b, ld_m, ld_out, S;
  int T;
  bq_spike_fade_params p;
  uint8_t* st_active;
  int64_t* st_ot;
  double *st_high, *st_close;
  uint8_t *event, *detail, *bars;
};

struct SpikeFadeStep {
  double o, h, c;
  int64_t ot;
  uint8_t src, sm, fm;
};

__global__ __launch_bounds__(RP_NT) void spike_fade_kernel(const SpikeFadeArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const int W = A.p.window_bars;
  const double ef = A.p.ext_factor;
  const double* __restrict__ op = A.open + s * A.ld_in;
  const double* __restrict__ hi = A.high + s * A.ld_in;
  const double* __restrict__ cl = A.close + s * A.ld_in;
  const int64_t* __restrict__ ts = A.ts + s * A.ld_ts;
  const uint8_t* __restrict__ so = A.source + s * A.ld_b;
  const uint8_t* __restrict__ sm = A.src_market ? A.src_market + s * A.ld_m : nullptr;
  const uint8_t* __restrict__ fm = A.fail_market ? A.fail_market + s * A.ld_m : nullptr;
  uint8_t* __restrict__ ev_out = A.event + s * A.ld_out;
  uint8_t* __restrict__ dt_out = A.detail ? A.detail + s * A.ld_out : nullptr;
  uint8_t* __restrict__ br_out = A.bars ? A.bars + s * A.ld_out : nullptr;

  // the row's state: wave-uniform from here on
  bool active = A.st_active && A.st_active[s] != 0;
  int64_t p_ot = active ? A.st_ot[s] : 0;
  double p_hi = active ? A.st_high[s] : qnan(), p_cl = active ? A.st_close[s] : qnan();
  int p = 0;                // the pending spike's candle
  bool lost = false;        // a carried-in spike that is not in [first, from]
  bool ext_carry = false;   // a carried-in spike: some high in (p, from) extends beyond it
  if (active && R.any()) {
    lost = true;
    for (int top = from; top >= first; top -= WAVE) {   // candles top, top - 1, ...: lane 0 is the newest
      const int u = top - lane;
      const bool in = u >= first;
      const int64_t v = in ? ts[u] : 0;
      const uint64_t hit = __ballot(in && v == p_ot);
      if (hit) {
        p = top - __builtin_ctzll(hit);
        lost = false;
        break;
      }
      if (__ballot(in && v < p_ot)) break;   // ascending: nothing older can match
    }
    if (!lost && from - p >= 2 && from - p <= W) {   // candles p + 1 .. from - 1 (W <= 32 of them: one load)
      const int u = from - 1 - lane;
      ext_carry = __ballot(u > p && hi[u] > p_hi * ef) != 0;
    }
  }

  const int b0 = R.b0();
  // one step's columns, candle tb + lane (NaN / 0 past the row's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    SpikeFadeStep x;
    x.o = in ? op[u] : qnan();
    x.h = in ? hi[u] : qnan();
    x.c = in ? cl[u] : qnan();
    x.ot = in ? ts[u] : 0;
    x.src = in ? so[u] : 0;
    x.sm = sm ? (in ? sm[u] : 0) : 1;
    x.fm = fm ? (in ? fm[u] : 0) : 1;
    return x;
  };
  SpikeFadeStep nxt = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!R.any() || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) {
        ev_out[t] = BQ_FS_NO_FRAME;
        if (dt_out) dt_out[t] = 0;
        if (br_out) br_out[t] = 0;
      }
      continue;
    }
    if (t0 == b0) nxt = load_step(t0);
    const SpikeFadeStep cur = nxt;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's walk
    const double o = cur.o, h = cur.h, c = cur.c;
    const int64_t ot = cur.ot;
    const bool src = cur.src != 0, smk = cur.sm != 0, fmk = cur.fm != 0;
    const bool valid = t >= from && t < len;
    const uint64_t V = __ballot(valid);
    const uint64_t SRC = __ballot(src && smk) & V;   // :618-621
    int ev = valid ? BQ_FS_IDLE : BQ_FS_NO_FRAME;
    int dt = valid ? (src ? 0 : BQ_FS_D_SOURCE) | (smk ? 0 : BQ_FS_D_MARKET) : 0;   // :638-646
    int br = 0;
    int pos = 0;   // candles before lane `pos` are decided
    while (pos < WAVE) {
      const uint64_t rest = V & (~0ull << pos);
      if (!rest) break;
      if (!active) {
        const uint64_t m = SRC & rest;
        if (!m) break;   // idle to the end of the step
        const int i = __builtin_ctzll(m);
        p_ot = readlane_i64(ot, i);   // _set_pending_spike (:622-630)
        p_hi = readlane_f64(h, i);
        p_cl = readlane_f64(c, i);
        p = t0 + i;
        active = true;
        if (lane == i) {
          ev = BQ_FS_SOURCE_SET;
          dt = 0;
        }
        pos = i + 1;
      } else if (lost) {   // :652-655: the first replayed candle, consumed
        const int i = __builtin_ctzll(rest);
        if (lane == i) {
          ev = BQ_FS_CLEARED;
          dt = BQ_FS_D_CANDLE_EXPIRED;
        }
        lost = false;
        active = false;
        pos = i + 1;
      } else {
        const int bars = t - p;   // > 0 except on a carried-in spike's own candle (:660-661)
        const double thr = p_hi * ef;
        const bool after = valid && bars > 0;
        const bool fnh = h >= p_hi && c < o && c < p_cl;                 // :679-683
        const uint64_t XW = __ballot(after && bars > W) & rest;          // :662
        const uint64_t XE = __ballot(after && (h > thr || (ext_carry && t == from))) & rest;   // :667-672
        const uint64_t C = __ballot(after && fnh && fmk) & rest;         // :685, :695
        const uint64_t any = XW | XE | C;
        const int end = any ? __builtin_ctzll(any) : WAVE;
        if (valid && lane >= pos && lane <= end) {   // the spike is pending on this candle
          const uint64_t bit = 1ull << lane;
          br = bars > 255 ? 255 : bars > 0 ? bars : 0;
          if (lane < end) {
            ev = bars > 0 ? BQ_FS_WAITING : BQ_FS_SAME_CANDLE;
            dt = bars > 0 ? (fnh ? 0 : BQ_FS_D_NEW_HIGH) | (fmk ? 0 : BQ_FS_D_MARKET) : 0;
          } else {
            ev = (XW | XE) & bit ? BQ_FS_CLEARED : BQ_FS_CANDIDATE;
            dt = XW & bit ? BQ_FS_D_WINDOW_EXPIRED : XE & bit ? BQ_FS_D_EXTENSION : 0;
          }
        }
        if (end == WAVE) break;   // still pending at the step's end
        active = false;           // _clear_pending_spike: the candle is consumed (:663, :673, :695)
        pos = end + 1;
      }
    }
    if (t < T) {
      ev_out[t] = (uint8_t)ev;
      if (dt_out) dt_out[t] = (uint8_t)dt;
      if (br_out) br_out[t] = (uint8_t)br;
    }
  }
  if (A.st_active && lane == 0) {
    A.st_active[s] = active ? 1 : 0;
    A.st_ot[s] = active ? p_ot : 0;
    A.st_high[s] = active ? p_hi : qnan();
    A.st_close[s] = active ? p_cl : qnan();
  }
}

}  // namespace bq

extern "C" void bq_spike_fade_default_params(bq_spike_fade_params* p) {
  if (!p) return;
  // FailedSpikeFade's class attributes (:42-43)
  p->window_bars = 8;
  p->ext_factor = 1 + 0.06;   // 1 + MAX_POST_SPIKE_EXTENSION (:670-672)
}

extern "C" int bq_spike_fade_replay(const double* open, const double* high, const double* close, int64_t ld_in,
                                    const int64_t* open_time, int64_t ld_ts, const uint8_t* source_ok, int64_t ld_b,
                                    const uint8_t* src_market, const uint8_t* fail_market, int64_t ld_m,
                                    const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S,
                                    int64_t T, const bq_spike_fade_params* params, uint8_t* st_active,
                                    int64_t* st_open_time, double* st_high, double* st_close, uint8_t* event,
                                    uint8_t* detail, uint8_t* bars, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!open || !high || !close || !open_time || !source_ok || !event || S < 0 || T < 0 || ld_in < T || ld_ts < T ||
      ld_b < T || ld_out < T || (ld_m != 0 && ld_m < T) || T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  const int nstate = (st_active != nullptr) + (st_open_time != nullptr) + (st_high != nullptr) + (st_close != nullptr);
  if (nstate != 0 && nstate != 4) return BQ_EINVAL;
  SpikeFadeArgs A;
  if (params) A.p = *params;
  else bq_spike_fade_default_params(&A.p);
  if (A.p.window_bars < 1 || A.p.window_bars > BQ_SPIKEFADE_MAX_WINDOW || !all_finite({A.p.ext_factor}))
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.open = open;
  A.high = high;
  A.close = close;
  A.ts = open_time;
  A.source = source_ok;
  A.src_market = src_market;
  A.fail_market = fail_market;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_in = ld_in;
  A.ld_ts = ld_ts;
  A.ld_b = ld_b;
  A.ld_m = ld_m;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.st_active = st_active;
  A.st_ot = st_open_time;
  A.st_high = st_high;
  A.st_close = st_close;
  A.event = event;
  A.detail = detail;
  A.bars = bars;
  hipLaunchKernelGGL(spike_fade_kernel, dim3((unsigned)blocks), dim3(RP_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
