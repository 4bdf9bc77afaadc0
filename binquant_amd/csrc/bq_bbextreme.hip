// BBExtremeReversion.signal() replayed over a [S][T] panel of 15m frames
// (gfx950; strategies/coinrule/bb_extreme_reversion.py:234-285 with evaluate
// :152-232 and _compute_rsi :134-150): the frame gate, the null gate over the
// last `lookback` closes, the RSI of that frame, the band position and the two
// extremes. Column t of row s = the method on the message whose frame is
// df.iloc[first_t[s]:t + 1] with current_price = close[t] and the bands of
// candle t; the method keeps no state (the rule table: include/binquant_amd.h).
//
// bb_extreme_kernel: the wave-per-row replay mapping (bq_replay.h).
//   1. the RSI is local to the frame: gain / loss .rolling(rsi_window).mean()
//      over df.tail(lookback) is pandas' roll_mean (2.3.3,
//      _libs/window/aggregations.pyx), an online add / remove sum with one
//      Kahan compensation for the adds and one for the removes, started at the
//      frame's first row. Its last value depends on all `lookback` closes, so
//      every lane replays the chain of its own candle: lookback - 1 dependent
//      steps for the two series, with the consecutive-same-value rule, the two
//      sign rules and +-inf as a missing observation.
//   2. the chain's inputs are the gains and losses of the close differences,
//      the same for every frame that holds both candles (the frame's first row
//      is the constant 0.0 / -0.0): each step writes its 64 gains and losses to
//      two 128-entry rings in LDS (this step and the one before, 2 KiB a wave;
//      lookback <= 64) and a lane reads g[t - k] / q[t - k] from them, one
//      ds_read_b64 per value and conflict-free. The lane-move form costs four
//      ds_bpermute_b32 and a select per value on the same LDS crossbar, with
//      both steps' values held in registers. lane 0's difference takes the
//      previous step's lane 63 through a readlane: close is loaded once per
//      candle.
//   3. the chain is bound by VALU issue, not by memory, so a
//      wave whose two steps hold no infinite difference (a ballot, carried)
//      runs the chain as the two Kahan sums alone, 16 fp64 operations a row:
//      with every row an observation, prev_value, the run of equal values and
//      neg_ct are functions of the last rsi_window rows and are formed from
//      them after the chain. Otherwise pandas' state is carried row by row.
//   4. the null gate's look-back is two ballots: this step's NaN closes and the
//      previous step's (wave-uniform, carried).
//   The step before from_t's loads close alone (the rings and the ballots).
//   32 B in (close and the three bands) and 1 + 5 x 8 B out per candle; no
//   atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3): 70 VGPRs, 74 SGPRs, 7 waves /
//   SIMD, no spills, scratch 0, LDS 8192 B a workgroup (4 waves x 2 x 128 x
//   8 B). The all-observed chain's loop is 22 VALU instructions a row (16
//   fp64) and two LDS reads of two values.
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

constexpr int BBX_RING = 2 * WAVE;

struct BbxArgs {
  const double *close, *up, *mid, *lo;
  const int64_t *lens, *first, *from;
  int64_t ld_px, ld_bb, ld_out, S;
  int T, omask;
  bq_bb_extreme_params p;
  uint8_t* status;
  double* val[BQ_BBX_NVALUES];
};

struct BbxStep {
  double c, u, m, l;   // close, bb_upper, bb_mid, bb_lower at candle t
};

// pandas' roll_mean state (add_mean / remove_mean / calc_mean), for a wave that has a +-inf difference in reach
struct RollMean {
  double sum, ca, cr, prev;   // sum_x, compensation_add, compensation_remove, prev_value
  int nobs, neg, same;        // nobs, neg_ct, num_consecutive_same_value

  // the state after the frame's first row v0 (0.0 for the gains, -0.0 for the losses: 0.0 + -0.0 = 0.0)
  __device__ __forceinline__ void start(double v0, bool negative) {
    sum = ca = cr = 0.0;
    prev = v0;
    nobs = same = 1;
    neg = negative ? 1 : 0;
  }
  __device__ __forceinline__ void add(double v) {
    if (win_ok(v)) {   // +-inf is NaN to the window (_prep_values)
      nobs += 1;
      const double y = v - ca;
      const double t = sum + y;
      ca = t - sum - y;
      sum = t;
      neg += __builtin_signbit(v) ? 1 : 0;
      same = v == prev ? same + 1 : 1;
      prev = v;
    }
  }
  __device__ __forceinline__ void remove(double v) {
    if (win_ok(v)) {
      nobs -= 1;
      const double y = -v - cr;
      const double t = sum + y;
      cr = t - sum - y;
      sum = t;
      neg -= __builtin_signbit(v) ? 1 : 0;
    }
  }
  __device__ __forceinline__ double mean(int minp) const {
    if (!(nobs >= minp && nobs > 0)) return qnan();
    double r = sum / (double)nobs;
    if (same >= nobs) r = prev;
    else if (neg == 0 && r < 0.0) r = 0.0;
    else if (neg == nobs && r > 0.0) r = 0.0;
    return r;
  }
};

// delta.where(delta > 0, 0.0) and -delta.where(delta < 0, 0.0): a NaN delta is 0.0 / -0.0
__device__ __forceinline__ double bbx_gain(double d) { return d > 0.0 ? d : 0.0; }
__device__ __forceinline__ double bbx_loss(double d) { return -(d < 0.0 ? d : 0.0); }

// _compute_rsi :140-144 on the frame whose row j is candle base + j, 1 <= W < L: the unclamped RSI, NaN for None.
// rg / rq: the rings of gains and losses by candle; the frame's first row is 0.0 / -0.0 whatever the ring holds.
__device__ __forceinline__ double bbx_frame_rsi(const double* rg, const double* rq, int base, int L, int W) {
  RollMean G, Q;
  G.start(0.0, false);
  Q.start(-0.0, true);
  for (int j = 1; j < W; ++j) {   // the windows still growing: adds alone
    G.add(rg[(base + j) & (BBX_RING - 1)]);
    Q.add(rq[(base + j) & (BBX_RING - 1)]);
  }
  for (int j = W; j < L; ++j) {   // pandas removes row j - W, then adds row j
    const bool head = j == W;
    const double gr = rg[(base + j - W) & (BBX_RING - 1)], qr = rq[(base + j - W) & (BBX_RING - 1)];
    G.remove(head ? 0.0 : gr);
    Q.remove(head ? -0.0 : qr);
    G.add(rg[(base + j) & (BBX_RING - 1)]);
    Q.add(rq[(base + j) & (BBX_RING - 1)]);
  }
  const double rs = G.mean(W) / Q.mean(W);
  return 100.0 - (100.0 / (1.0 + rs));   // :143-144
}

// Kahan's step as add_mean / remove_mean write it (remove passes -v)
__device__ __forceinline__ void bbx_kahan(double v, double& sum, double& comp) {
  const double y = v - comp;
  const double t = sum + y;
  comp = t - sum - y;
  sum = t;
}

// The same where no difference in reach of the wave is infinite: every row is an observation, nobs is W from row
// W - 1 on, and what calc_mean reads besides the sum (prev_value, the run of equal values, neg_ct) is a function
// of the last W rows alone: it is formed from them after the chain, not carried through it. The chain is then
// the two Kahan sums: 16 fp64 operations and four ring reads a row.
__device__ __forceinline__ double bbx_frame_rsi_all_observed(const double* rg, const double* rq, int base, int L,
                                                             int W) {
  double gs = 0.0, gca = 0.0, gcr = 0.0, qs = 0.0, qca = 0.0, qcr = 0.0;   // after the first row: 0.0 + -0.0 = 0.0
  for (int j = 1; j < W; ++j) {
    bbx_kahan(rg[(base + j) & (BBX_RING - 1)], gs, gca);
    bbx_kahan(rq[(base + j) & (BBX_RING - 1)], qs, qca);
  }
  bbx_kahan(-0.0, gs, gcr);   // row W removes the frame's first row: -(0.0) and -(-0.0)
  bbx_kahan(0.0, qs, qcr);
  bbx_kahan(rg[(base + W) & (BBX_RING - 1)], gs, gca);
  bbx_kahan(rq[(base + W) & (BBX_RING - 1)], qs, qca);
  for (int j = W + 1; j < L; ++j) {
    bbx_kahan(-rg[(base + j - W) & (BBX_RING - 1)], gs, gcr);
    bbx_kahan(-rq[(base + j - W) & (BBX_RING - 1)], qs, qcr);
    bbx_kahan(rg[(base + j) & (BBX_RING - 1)], gs, gca);
    bbx_kahan(rq[(base + j) & (BBX_RING - 1)], qs, qca);
  }
  // calc_mean over rows L - W .. L - 1 (none is the frame's first: W < L). A loss has the sign bit exactly where it
  // is -0.0: a loss is positive or -0.0, a gain positive or 0.0.
  const double gl = rg[(base + L - 1) & (BBX_RING - 1)], ql = rq[(base + L - 1) & (BBX_RING - 1)];
  bool gsame = true, qsame = true;
  int qneg = ql > 0.0 ? 0 : 1;
  for (int j = L - W; j < L - 1; ++j) {
    const double g = rg[(base + j) & (BBX_RING - 1)], q = rq[(base + j) & (BBX_RING - 1)];
    gsame = gsame && g == gl;
    qsame = qsame && q == ql;
    qneg += q > 0.0 ? 0 : 1;
  }
  double gm = gs / (double)W, qm = qs / (double)W;
  if (gsame) gm = gl;
  else if (gm < 0.0) gm = 0.0;   // neg_ct == 0
  if (qsame) qm = ql;
  else if (qneg == 0 && qm < 0.0) qm = 0.0;
  else if (qneg == W && qm > 0.0) qm = 0.0;
  return 100.0 - (100.0 / (1.0 + gm / qm));   // :143-144
}

__global__ __launch_bounds__(RP_NT) void bb_extreme_kernel(const BbxArgs A) {
  __shared__ double ring_all[RP_WPB][2][BBX_RING];   // gains, losses
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  double* rg = ring_all[__builtin_amdgcn_readfirstlane(threadIdx.x / WAVE)][0];
  double* rq = ring_all[__builtin_amdgcn_readfirstlane(threadIdx.x / WAVE)][1];
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const double* __restrict__ cl = A.close + s * A.ld_px;
  const double* __restrict__ up = A.up + s * A.ld_bb;
  const double* __restrict__ md = A.mid + s * A.ld_bb;
  const double* __restrict__ lw = A.lo + s * A.ld_bb;
  // omask bit k: a BQ_BBX_V_*
  ReplayOut<BbxArgs, BQ_BBX_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_BBX_NVALUES; ++k) O.set(k, A.val[k]);

  // one step's columns, candle tb + lane (NaN past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    BbxStep x;
    x.c = in ? cl[u] : qnan();
    x.u = in ? up[u] : qnan();
    x.m = in ? md[u] : qnan();
    x.l = in ? lw[u] : qnan();
    return x;
  };
  // The gains and losses of the step's differences close[t] - close[t - 1] into the rings (lane 0: against the
  // previous step's lane 63) and its NaN ballot; inf: a difference of the step is infinite; returns the step's lane 63 close. A wave reads only
  // what it wrote itself: LDS operations of a wave complete in order.
  auto ring_step = [&](double c, double c_last, int t0, uint64_t& NB, bool& inf) {
    const double cp = dpp_f64<DPP_WAVE_SHR1>(c);
    const double d = c - (lane ? cp : c_last);
    inf = __ballot(__builtin_isinf(d)) != 0;
    rg[(t0 + lane) & (BBX_RING - 1)] = bbx_gain(d);
    rq[(t0 + lane) & (BBX_RING - 1)] = bbx_loss(d);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    NB = __ballot(c != c);
    return readlane_f64(c, WAVE - 1);
  };

  const int b0 = R.b0();
  const bool any = R.any();
  uint64_t NBP = 0;        // the previous step's NaN closes
  bool infp = false;       // an infinite difference in the previous step
  double c_last = qnan();  // and its lane 63 close

  BbxStep cur = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) O.no_frame(t0, BQ_BBX_NO_FRAME);
      if (any && t0 + WAVE == b0) c_last = ring_step(t < T ? cl[t] : qnan(), qnan(), t0, NBP, infp);   // the step before
      continue;
    }
    if (t0 == b0) cur = load_step(t0);
    BbxStep nxt = cur;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's arithmetic
    const Karg<BbxArgs> K = kernarg<BbxArgs>();
    const int L = K->p.lookback, W = K->p.rsi_window;

    uint64_t NB;
    bool inf;
    const double c_end = ring_step(cur.c, c_last, t0, NB, inf);
    const bool valid = t >= from && t < len;
    const bool enough = t + 1 - first >= L;                // :255
    const bool nulls = window_hit(NB, NBP, L, lane);       // :264 over df.tail(lookback)
    const bool reached = valid && enough && !nulls;

    // ---- _compute_rsi on the frame's last `lookback` closes: row j of the frame is candle t - (L - 1) + j
    double rsi = qnan();
    if (W < L && __ballot(reached))   // :138 len(closes) >= window + 1; wave-uniform, as is the choice of the chain
      rsi = inf || infp ? bbx_frame_rsi(rg, rq, t - (L - 1), L, W)
                        : bbx_frame_rsi_all_observed(rg, rq, t - (L - 1), L, W);
    const bool no_rsi = rsi != rsi;                              // :146
    const double rsi_value = py_max(0.0, py_min(100.0, rsi));    // :150

    // ---- evaluate :161-170
    const auto& P = K->p;
    const double span = cur.u - cur.l;
    const double pos = span > 0.0 ? (cur.c - cur.l) / span : 0.5;
    const double width = cur.m > 0.0 ? span / cur.m : 0.0;
    const double dist = cur.m > 0.0 ? (cur.c - cur.m) / cur.m * 100.0 : 0.0;
    const bool buy = rsi_value <= P.oversold_rsi && pos <= P.max_lower_band_position;       // :194
    const bool sell = rsi_value >= P.overbought_rsi && pos >= P.min_upper_band_position;    // :209

    int st = BQ_BBX_EMIT;
    if (!valid) st = BQ_BBX_NO_FRAME;
    else if (!enough) st = BQ_BBX_NOT_ENOUGH_DATA;
    else if (nulls) st = BQ_BBX_NULLS;
    else if (no_rsi) st = BQ_BBX_NO_RSI;
    else if (span <= 0.0) st = BQ_BBX_INVALID_BAND;   // :187, a NaN span goes on
    else if (!buy && !sell) st = BQ_BBX_NO_EXTREME;

    if (t < T) {
      O.st[t0] = (uint8_t)st;
      if (O.has(BQ_BBX_V_RSI)) O.val[BQ_BBX_V_RSI][t0] = reached ? (no_rsi ? 50.0 : rsi_value) : qnan();
      if (O.has(BQ_BBX_V_POSITION)) O.val[BQ_BBX_V_POSITION][t0] = reached ? pos : qnan();
      if (O.has(BQ_BBX_V_WIDTH)) O.val[BQ_BBX_V_WIDTH][t0] = reached ? width : qnan();
      if (O.has(BQ_BBX_V_DISTANCE)) O.val[BQ_BBX_V_DISTANCE][t0] = reached ? dist : qnan();
      if (O.has(BQ_BBX_V_DIRECTION))
        O.val[BQ_BBX_V_DIRECTION][t0] = st == BQ_BBX_EMIT ? (buy ? (double)BQ_DIR_LONG : (double)BQ_DIR_SHORT) : qnan();
    }
    NBP = NB;
    infp = inf;
    c_last = c_end;
    cur = nxt;
  }
}

}  // namespace bq

extern "C" void bq_bb_extreme_default_params(bq_bb_extreme_params* p) {
  if (!p) return;
  // BBExtremeReversion's class attributes (:50-55, :67)
  p->lookback = 30;
  p->rsi_window = 2;
  p->oversold_rsi = 5.0;
  p->overbought_rsi = 95.0;
  p->max_lower_band_position = 0.0;
  p->min_upper_band_position = 1.0;
}

extern "C" int bq_bb_extreme_replay(const double* close, int64_t ld_px, const double* bb_upper, const double* bb_mid,
                                    const double* bb_lower, int64_t ld_bb, const int64_t* lens, const int64_t* first_t,
                                    const int64_t* from_t, int64_t S, int64_t T, const bq_bb_extreme_params* params,
                                    uint8_t* status, double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  if (!close || !bb_upper || !bb_mid || !bb_lower || !status || S < 0 || T < 0 || ld_px < T || ld_bb < T ||
      ld_out < T || T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  BbxArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_bb_extreme_default_params(&A.p);
  const bq_bb_extreme_params& p = A.p;
  if (!all_finite({p.oversold_rsi, p.overbought_rsi, p.max_lower_band_position, p.min_upper_band_position}))
    return BQ_EINVAL;
  if (p.lookback < 1 || p.lookback > BQ_BBX_MAX_LOOKBACK || p.rsi_window < 1) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.close = close;
  A.up = bb_upper;
  A.mid = bb_mid;
  A.lo = bb_lower;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_px = ld_px;
  A.ld_bb = ld_bb;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.status = status;
  replay_values(A.val, A.omask, values);
  hipLaunchKernelGGL(bb_extreme_kernel, dim3((unsigned)blocks), dim3(RP_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
