// Entry gates of two wired 15m strategies at every prefix of a [S][T] panel
// (gfx950): column t of row s = the method on the frame df.iloc[first:t + 1],
// first = first_t[s] (the rows Candles.post_process dropped; NULL: 0).
//
// impulse_kernel: RelativeStrengthImpulseRider._features
//   (strategies/relative_strength_impulse_rider.py:92-198) with _btc_return_at
//   (:69-90): a 7-candle stencil over open / high / low / close / ATR, the
//   benchmark return joined on the trigger's open_time, and the 15-step
//   ordered gate. One workgroup per (symbol, IR_TILE-candle tile), a thread
//   per candle (IR_CPT candles, strided by the block):
//   1. the tile's closes with the 6 candles before it in LDS (five reads per
//      candle); the trigger's open, ATR and open time are the neighbouring
//      lane's candle, re-read through L1 (staging them too costs 32 KiB of
//      LDS a block, 4 waves per SIMD instead of 8: 1.08 against 0.85 ms at
//      12.5k x 2k);
//   2. per candle t (trigger tr = t - 1, confirmation cf = t): the benchmark
//      row of open_time[tr] (bq_bench_lookup.h) and the row four POSITIONS
//      before it, every derived value with the reference's own expression
//      (one or two correctly rounded fp64 operations each: bit-exact), every
//      predicate, and the status as a priority encode of selects (no ladder
//      of per-lane branches) — the first failing check in the reference's
//      order, 0 = confirmed. Values are NaN where the status is not 0 (the
//      method returns None there).
//   Inputs cross HBM once (the halos re-read L2); nothing but the outputs is
//   written: 48 B in + 73 B out per candle with every column requested.
//
// bb_stable_kernel: LadderDeployer._bb_stable (strategies/grid/ladder_deployer.py
//   :42-56): the last n rows all have bb_mid > 0 and width = (upper - lower) /
//   mid > 0, and |w[t] - w[t-n+1]| / w[t-n+1] * 100 <= max_change_pct. The
//   widths and a bad-row bitmask (a wave ballot per 64 candles) of the tile
//   and the 64 candles before it go to LDS; "all n rows valid" is a popcount
//   of the window's mask bits, not a walk (bq_bbwalk.h, shared with
//   bq_ladder.hip).
#include "bq_bbwalk.h"
#include "bq_bench_lookup.h"
#include "bq_candletile.h"
#include "bq_device.h"
#include "binquant_amd.h"

namespace bq {

constexpr int IR_TILE = CT_TILE, IR_NT = CT_NT, IR_CPT = CT_CPT;   // the kernel's names for the geometry
constexpr int IR_HC = 8;   // close slots before the tile (the stencil reaches t - 6)

struct ImpulseArgs {
  const double *open, *high, *low, *close, *atr;
  const int64_t* ts;
  const int64_t *lens, *first;
  const int64_t* bts;
  const double* bclose;
  int64_t ld_in, ld_atr, ld_ts, ld_out;
  int T, nb, tiles;
  bq_impulse_params p;
  uint8_t* status;
  double* val[BQ_IR_NVALUES];
};

__device__ __forceinline__ bool pos_finite(double x) { return x > 0.0 && x < __builtin_inf(); }

__global__ __launch_bounds__(IR_NT) void impulse_kernel(const ImpulseArgs A) {
  __shared__ double sC[IR_HC + IR_TILE];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x / A.tiles;
  const int t0 = (int)(blockIdx.x % A.tiles) * IR_TILE;
  const int T = A.T;
  const double* __restrict__ cl = A.close + s * A.ld_in;
  const double* __restrict__ op = A.open + s * A.ld_in;
  const double* __restrict__ at = A.atr + s * A.ld_atr;
  const int64_t* __restrict__ ts = A.ts + s * A.ld_ts;
  // 1. the tile's closes and the IR_HC before it (NaN outside the row: such
  //    slots are read only by candles whose status is history_too_short)
  for (int i = tid; i < IR_HC + IR_TILE; i += IR_NT) {
    const int t = t0 - IR_HC + i;
    sC[i] = t >= 0 && t < T ? cl[t] : qnan();
  }
  __syncthreads();
  const int64_t len64 = A.lens ? A.lens[s] : (int64_t)T;
  const int len = len64 < 0 ? 0 : len64 > T ? T : (int)len64;
  const int64_t f64 = A.first ? A.first[s] : 0;
  const int first = f64 < 0 ? 0 : f64 > T ? T : (int)f64;
  const bool bench = A.nb >= 5;   // len(btc_df) < 5 (:71)
  const int64_t bt0 = bench ? A.bts[0] : 0;
  const int64_t bstep = bench ? bench_step(A.bts, A.nb, bt0) : 0;
  const bq_impulse_params P = A.p;
  const double* __restrict__ hi = A.high + s * A.ld_in;
  const double* __restrict__ lo = A.low + s * A.ld_in;
#pragma unroll
  for (int q = 0; q < IR_CPT; ++q) {
    const int u = q * IR_NT + tid, t = t0 + u;
    if (t >= T) continue;
    const int64_t o = s * A.ld_out + t;
    const int kc = IR_HC + u;   // candle t's close slot
    const double c_cf = sC[kc], c_tr = sC[kc - 1], c_pv = sC[kc - 2], a_imp = sC[kc - 5], a_prev = sC[kc - 6];
    // the trigger's open, ATR and open time: the neighbouring lane's candle,
    // re-read through L1 (candle 0 has no trigger: its status is history_too_short)
    const int tr = t > 0 ? t - 1 : 0;
    const double o_cf = op[t], o_tr = op[tr], atr = at[tr];
    const int64_t key = ts[tr];
    const double h_cf = hi[t], l_cf = lo[t];
    // _btc_return_at (:69-90): the last row at the trigger's time, its anchor
    // four positions before it in the benchmark frame
    double bc = qnan(), ba = qnan();
    int p = -1;
    if (bench && t >= 1) p = bench_last_match(A.bts, A.bclose, A.nb, key, bt0, bstep, bc);
    if (p >= 4) ba = A.bclose[p - 4];
    const double btc = bc / ba - 1.0;
    // a NaN close passes "anchor <= 0 or close <= 0" (:87); its return is not finite (:90)
    const bool f_btc = !(p >= 4) || ba <= 0.0 || bc <= 0.0 || !is_finite(btc);
    // the reference's expressions, in its operation order (:133-148, :180, :191)
    const double impulse = c_tr / a_imp - 1.0;
    const double previous = c_pv / a_prev - 1.0;
    const double rs = impulse - btc;
    const double atr_pct = atr / c_tr;
    const double conf_ret = c_cf / o_cf - 1.0;
    const double range = h_cf - l_cf;
    const double location = (c_cf - l_cf) / range;
    const double trig_ret = c_tr / o_tr - 1.0;
    const double entry = c_cf * P.entry_factor;
    // every check (:99-178)
    const bool f_short = t + 1 - first < P.min_history;
    const bool f_vals = !(pos_finite(c_tr) && pos_finite(o_tr) && pos_finite(o_cf) && pos_finite(h_cf) &&
                          pos_finite(l_cf) && pos_finite(c_cf) && pos_finite(atr));
    const bool f_anchor = a_imp <= 0.0 || a_prev <= 0.0 || c_pv <= 0.0;
    const bool f_range = range <= 0.0;
    const bool f_derived = !(is_finite(impulse) && is_finite(previous) && is_finite(btc) && is_finite(rs) &&
                             is_finite(atr_pct) && is_finite(conf_ret) && is_finite(location));
    const bool f_imp = !(P.min_impulse <= impulse && impulse <= P.max_impulse);
    const bool f_cross = previous >= P.min_impulse;
    const bool f_btc_hi = btc > P.max_btc_return;
    const bool f_rs = rs < P.min_rs;
    const bool f_atr = atr_pct > P.max_atr_pct;
    const bool f_hold = c_cf < c_tr;
    const bool f_conf = conf_ret < P.min_conf_return;
    const bool f_loc = location < P.min_close_location;
    // the first failing check: selects from the last check to the first
    int st = BQ_IR_CONFIRMED;
    st = f_loc ? BQ_IR_CLOSE_NOT_NEAR_HIGH : st;
    st = f_conf ? BQ_IR_CONFIRMATION_NEGATIVE : st;
    st = f_hold ? BQ_IR_DID_NOT_HOLD : st;
    st = f_atr ? BQ_IR_ATR_TOO_HIGH : st;
    st = f_rs ? BQ_IR_RS_TOO_LOW : st;
    st = f_btc_hi ? BQ_IR_BTC_TOO_HIGH : st;
    st = f_cross ? BQ_IR_DID_NOT_CROSS : st;
    st = f_imp ? BQ_IR_IMPULSE_RANGE : st;
    st = f_derived ? BQ_IR_NOT_READY : st;
    st = f_range ? BQ_IR_RANGE_INVALID : st;
    st = f_btc ? BQ_IR_BTC_UNAVAILABLE : st;
    st = f_anchor ? BQ_IR_INVALID_ANCHORS : st;
    st = f_vals ? BQ_IR_INVALID_VALUES : st;
    st = f_short ? BQ_IR_SHORT_HISTORY : st;
    st = t >= len ? BQ_IR_NO_FRAME : st;
    A.status[o] = (uint8_t)st;
    const bool ok = st == BQ_IR_CONFIRMED;
    const double v[BQ_IR_NVALUES] = {impulse, previous, btc, rs, trig_ret, conf_ret, location, atr_pct, entry};
#pragma unroll
    for (int k = 0; k < BQ_IR_NVALUES; ++k)
      if (A.val[k]) A.val[k][o] = ok ? v[k] : qnan();   // wave-uniform: a NULL column is skipped
  }
}

// ---- LadderDeployer._bb_stable ------------------------------------------------
constexpr int BS_TILE = CT_TILE, BS_NT = CT_NT, BS_CPT = CT_CPT;
constexpr int BS_H = WAVE;   // slots before the tile (n <= 64 reaches t - 63)
static_assert(BS_H % WAVE == 0 && BQ_BB_STABLE_MAX_N <= BS_H, "mask words are whole waves of slots");

struct StableArgs {
  const double *upper, *mid, *lower;
  const int64_t *lens, *first;
  int64_t ld_in, ld_out;
  int T, n, tiles;
  double max_change;
  uint8_t* stable;
  double* change;
};

__global__ __launch_bounds__(BS_NT) void bb_stable_kernel(const StableArgs A) {
  __shared__ double sW[BS_H + BS_TILE];
  __shared__ uint64_t sBad[(BS_H + BS_TILE) / WAVE];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x / A.tiles;
  const int t0 = (int)(blockIdx.x % A.tiles) * BS_TILE;
  const int T = A.T, n = A.n;
  const double* __restrict__ up = A.upper + s * A.ld_in;
  const double* __restrict__ md = A.mid + s * A.ld_in;
  const double* __restrict__ lw = A.lower + s * A.ld_in;
  // widths and bad rows of candles t0 - BS_H .. t0 + BS_TILE - 1: mid <= 0, or
  // width <= 0 (:49-53; a NaN row passes both tests). Slots outside the row
  // are read only by candles that return before the walk (len(df) < n).
  for (int i = tid; i < BS_H + BS_TILE; i += BS_NT) {
    double w;
    const bool bad = bb_slot(up, md, lw, t0 - BS_H + i, T, w);
    sW[i] = w;
    const uint64_t bm = __ballot(bad);   // slots i - lane .. i - lane + 63 (BS_NT % 64 == 0)
    if ((tid & (WAVE - 1)) == 0) sBad[i / WAVE] = bm;
  }
  __syncthreads();
  const int64_t len64 = A.lens ? A.lens[s] : (int64_t)T;
  const int len = len64 < 0 ? 0 : len64 > T ? T : (int)len64;
  const int64_t f64 = A.first ? A.first[s] : 0;
  const int first = f64 < 0 ? 0 : f64 > T ? T : (int)f64;
#pragma unroll
  for (int q = 0; q < BS_CPT; ++q) {
    const int u = q * BS_NT + tid, t = t0 + u;
    if (t >= T) continue;
    const int k = BS_H + u;   // the window's slots k - (n - 1) .. k (>= 1)
    const BbWindow win = bb_window(k, n);
    const int nbad = BQ_BB_WINDOW_BAD(sBad, win);
    const bool reached = t < len && t + 1 - first >= n && nbad == 0;   // change_pct is computed (:55)
    const double change = bb_change(sW[win.lo], sW[k]);
    const int64_t o = s * A.ld_out + t;
    A.stable[o] = reached && change <= A.max_change ? 1 : 0;
    if (A.change) A.change[o] = reached ? change : qnan();
  }
}

}  // namespace bq

extern "C" void bq_impulse_default_params(bq_impulse_params* p) {
  if (!p) return;
  // RelativeStrengthImpulseRider's class attributes (:36-46)
  p->min_impulse = 0.05;
  p->max_impulse = 0.18;
  p->min_rs = 0.08;
  p->max_btc_return = 0.01;
  p->min_conf_return = 0.0;
  p->min_close_location = 0.70;
  p->max_atr_pct = 0.06;
  p->entry_factor = 1 - 1.0 / 100;   // 1 - RETEST_DISCOUNT_PCT / 100 (:180)
  p->min_history = 20;
  p->reserved = 0;
}

extern "C" int bq_impulse_rider(const double* open, const double* high, const double* low, const double* close,
                                int64_t ld_in, const double* atr, int64_t ld_atr, const int64_t* open_time,
                                int64_t ld_ts, const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T,
                                const int64_t* bench_ts, const double* bench_close, int64_t nb,
                                const bq_impulse_params* params, uint8_t* status, double* const* values,
                                int64_t ld_out, void* stream) {
  using namespace bq;
  if (!open || !high || !low || !close || !atr || !open_time || !status || S < 0 || T < 0 || ld_in < T ||
      ld_atr < T || ld_ts < T || ld_out < T || nb < 0 || nb > 0x7fffffff)
    return BQ_EINVAL;
  int64_t tiles;
  if (!candle_tiles(S, T, tiles) || (nb > 0 && (!bench_ts || !bench_close))) return BQ_EINVAL;
  ImpulseArgs A;
  if (params) A.p = *params;
  else bq_impulse_default_params(&A.p);
  if (A.p.min_history < 7) return BQ_EINVAL;   // the stencil reaches t - 6
  if (S == 0 || T == 0) return BQ_OK;
  A.open = open;
  A.high = high;
  A.low = low;
  A.close = close;
  A.atr = atr;
  A.ts = open_time;
  A.lens = lens;
  A.first = first_t;
  A.bts = bench_ts;
  A.bclose = bench_close;
  A.ld_in = ld_in;
  A.ld_atr = ld_atr;
  A.ld_ts = ld_ts;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.nb = (int)nb;
  A.tiles = (int)tiles;
  A.status = status;
  tile_values(A.val, values);
  hipLaunchKernelGGL(impulse_kernel, dim3((unsigned)(tiles * S)), dim3(IR_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

extern "C" int bq_bb_stable(const double* bb_upper, const double* bb_mid, const double* bb_lower, int64_t ld_in,
                            const int64_t* lens, const int64_t* first_t, int64_t S, int64_t T, int32_t n,
                            double max_change_pct, uint8_t* stable, double* change_pct, int64_t ld_out,
                            void* stream) {
  using namespace bq;
  int64_t tiles;
  if (!bb_upper || !bb_mid || !bb_lower || !stable || S < 0 || T < 0 || ld_in < T || ld_out < T || n < 1 ||
      n > BQ_BB_STABLE_MAX_N || !candle_tiles(S, T, tiles))
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  StableArgs A;
  A.upper = bb_upper;
  A.mid = bb_mid;
  A.lower = bb_lower;
  A.lens = lens;
  A.first = first_t;
  A.ld_in = ld_in;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.n = n;
  A.tiles = (int)tiles;
  A.max_change = max_change_pct;
  A.stable = stable;
  A.change = change_pct;
  hipLaunchKernelGGL(bb_stable_kernel, dim3((unsigned)(tiles * S)), dim3(BS_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
