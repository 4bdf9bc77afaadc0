// LadderDeployer.signal() replayed over a [S][T] panel of 15m frames (gfx950;
// strategies/grid/ladder_deployer.py:58-187): the grid-only policy, the market
// context and the symbol's snapshot entry, _bb_stable over the frame's last n
// rows, the price-inside-the-bands and range-width tests, and the numbers the
// deployment is built from (range_width_pct, the ATR breakout buffer,
// breakout_low / breakout_high). Column t of row s = the method on the message
// whose frame is df_15m.iloc[first_t[s]:t + 1] (the rule table:
// include/binquant_amd.h). The method keeps no state.
//
// grid_ladder_kernel: one workgroup per (row, GL_TILE-candle tile), a thread
// per candle (GL_CPT candles, strided by the block), bb_stable_kernel's mapping
// (bq_impulse.hip) with its walk (bq_bbwalk.h):
//   1. a tile none of whose candles is replayed (before max(from_t, first_t)
//      or past lens: with from_t = T - 1 every tile but the last) writes
//      NO_FRAME / NaN and loads nothing;
//   2. each thread loads its own candles' frame bands, keeps them in registers
//      and writes their width and bad-row ballot to LDS; wave 0 does the same
//      for the 64 candles before the tile (n <= 64 reaches t - 63). Where the
//      bands passed to signal() are the frame's own columns, the registers
//      serve the price and width tests too: each column is read once;
//   3. per candle: the window's popcount and change_pct from LDS, the context
//      of the candle's time (one coalesced read per tile and row; an L2 hit
//      after the first row), the symbol's entry, every predicate, and the
//      status as a priority encode of selects from the last check to the first
//      (no ladder of per-lane branches). Python's min / max are selects.
//   At most 7 x 8 B in (4 with the bands aliased; + 12 B of context per candle
//   time, + 21 B of symbol snapshot where it is per candle) and 1 + 5 x 8 B
//   out per candle; a NULL value column is skipped (wave-uniform).
#include "bq_bbwalk.h"
#include "bq_candletile.h"
#include "bq_replay.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

constexpr int GL_TILE = CT_TILE, GL_NT = CT_NT, GL_CPT = CT_CPT;   // the kernel's names for the geometry
constexpr int GL_H = WAVE;   // slots before the tile (n <= 64 reaches t - 63)
static_assert(GL_H == WAVE && BQ_BB_STABLE_MAX_N <= GL_H, "mask words are whole waves of slots; wave 0 fills the halo");

struct GlArgs {
  const double *close, *bbu, *bbm, *bbl;    // current_price; the frame's bands
  const double *high, *mid, *low;           // the bands as passed to signal()
  const uint8_t *policy_ok, *ctx_ok;
  const int8_t* regime;
  const double* score;
  const uint8_t *sym_ok, *sym_regime, *sym_transition, *sym_e20, *sym_e50;
  const double *sym_rs, *sym_atr;
  const int64_t *lens, *first, *from;
  int64_t ld_c, ld_bb, ld_bands, ld_sym, ld_out;
  int T, tiles, ctx_T, alias;
  bq_grid_ladder_params p;
  uint8_t* status;
  double* val[BQ_GL_NVALUES];
};

__global__ __launch_bounds__(GL_NT) void grid_ladder_kernel(const GlArgs A) {
  __shared__ double sW[GL_H + GL_TILE];
  __shared__ uint64_t sBad[(GL_H + GL_TILE) / WAVE];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x / A.tiles;
  const int t0 = (int)(blockIdx.x % A.tiles) * GL_TILE;
  const int T = A.T;
  const int64_t len64 = A.lens ? A.lens[s] : (int64_t)T;
  const int len = len64 < 0 ? 0 : len64 > T ? T : (int)len64;
  const int64_t f64 = A.first ? A.first[s] : 0;
  const int first = f64 < 0 ? 0 : f64 > T ? T : (int)f64;
  const int64_t r64 = A.from ? A.from[s] : 0;
  const int from = r64 < 0 ? 0 : r64 > T ? T : (int)r64;
  const int begin = from > first ? from : first;   // candles begin .. len - 1 are replayed
  const int64_t orow = s * A.ld_out;

  // 1. no replayed candle in the tile (workgroup-uniform)
  if (t0 >= len || t0 + GL_TILE <= begin) {
#pragma unroll
    for (int q = 0; q < GL_CPT; ++q) {
      const int t = t0 + q * GL_NT + tid;
      if (t >= T) continue;
      A.status[orow + t] = (uint8_t)BQ_GL_NO_FRAME;
#pragma unroll
      for (int k = 0; k < BQ_GL_NVALUES; ++k)
        if (A.val[k]) A.val[k][orow + t] = qnan();
    }
    return;
  }

  // 2. widths and bad rows of candles t0 - GL_H .. t0 + GL_TILE - 1 (:49-53). Slots outside the row are read only by
  //    candles that return before the walk (len(df) < n).
  const double* __restrict__ up = A.bbu + s * A.ld_bb;
  const double* __restrict__ md = A.bbm + s * A.ld_bb;
  const double* __restrict__ lw = A.bbl + s * A.ld_bb;
  if (tid < GL_H) {   // wave 0, whole
    double w;
    const bool bad = bb_slot(up, md, lw, t0 - GL_H + tid, T, w);
    sW[tid] = w;
    const uint64_t bm = __ballot(bad);
    if (tid == 0) sBad[0] = bm;
  }
  double fu[GL_CPT], fm[GL_CPT], fl[GL_CPT];
#pragma unroll
  for (int q = 0; q < GL_CPT; ++q) {
    const int u = q * GL_NT + tid, t = t0 + u;
    const bool in = t < T;
    fu[q] = in ? up[t] : qnan();
    fm[q] = in ? md[t] : qnan();
    fl[q] = in ? lw[t] : qnan();
    double w;
    const bool bad = bb_row(fu[q], fm[q], fl[q], w);   // NaN past the panel's end: width NaN, not bad
    sW[GL_H + u] = w;
    const uint64_t bm = __ballot(bad);   // slots GL_H + u - lane .. + 63 (GL_NT % 64 == 0)
    if ((tid & (WAVE - 1)) == 0) sBad[(GL_H + u) / WAVE] = bm;
  }
  __syncthreads();

  // 3. the method, candle by candle
  const bq_grid_ladder_params P = A.p;
  const int n = P.n;
  const double* __restrict__ cl = A.close + s * A.ld_c;
  const double* __restrict__ hp = A.high + s * A.ld_bands;
  const double* __restrict__ mp = A.mid + s * A.ld_bands;
  const double* __restrict__ lp = A.low + s * A.ld_bands;
#pragma unroll
  for (int q = 0; q < GL_CPT; ++q) {
    const int u = q * GL_NT + tid, t = t0 + u;
    if (t >= T) continue;
    // _bb_stable (:42-56) on the frame's columns
    const int k = GL_H + u;   // the window's slots k - (n - 1) .. k (>= 1)
    const BbWindow win = bb_window(k, n);
    const int nbad = BQ_BB_WINDOW_BAD(sBad, win);
    const bool reached = t + 1 - first >= n && nbad == 0;   // change_pct is computed (:55)
    const double change = bb_change(sW[win.lo], sW[k]);
    // the message's arguments
    const double price = cl[t];
    double high = fu[q], mid = fm[q], low = fl[q];
    if (!A.alias) {   // wave-uniform
      high = hp[t];
      mid = mp[t];
      low = lp[t];
    }
    // the context of the candle's time and the symbol's snapshot entry
    const int ci = A.ctx_T == 1 ? 0 : t;
    const bool pok = A.policy_ok ? A.policy_ok[ci] != 0 : true;
    const bool cok = A.ctx_ok ? A.ctx_ok[ci] != 0 : true;
    const int regime = A.regime[ci];
    const double score = A.score[ci];
    bool sok = false, e20 = false, e50 = false;
    int sreg = BQ_MR_NONE, strans = BQ_MR_NONE;
    double rs = 0.0, atr = 0.0;
    if (A.sym_ok) {   // wave-uniform
      const int64_t si = A.ld_sym ? s * A.ld_sym + t : s;
      sok = A.sym_ok[si] != 0;
      sreg = A.sym_regime[si];
      strans = A.sym_transition[si];
      e20 = A.sym_e20[si] != 0;
      e50 = A.sym_e50[si] != 0;
      rs = A.sym_rs[si];
      atr = A.sym_atr[si];
    }
    // the method's expressions, in its operation order (:112-124, :150-151)
    const double rw = mid > 0.0 ? ((high - low) / mid) * 100.0 : 0.0;
    const double raw = (atr * 100.0) * P.atr_multiplier;
    const double buf = py_max(P.min_buffer_pct, py_min(P.max_buffer_pct, raw));
    const double blow = low * (1.0 - buf / 100.0);
    const double bhigh = high * (1.0 + buf / 100.0);
    // every check (:70-119; compares in the method's direction: a NaN fails)
    const bool f_policy = !pok;
    const bool f_ctx = !cok;
    const bool f_range = regime != BQ_GL_REGIME_RANGE;
    const bool f_micro = !sok || sreg != BQ_GL_REGIME_RANGE;
    const bool f_trans = strans == BQ_GL_TRANSITION_BREAKDOWN || strans == BQ_GL_TRANSITION_VOLATILITY_EXPANSION ||
                         strans == BQ_GL_TRANSITION_ENTERED_TREND_DOWN;
    const bool f_ema = !e20 && !e50;
    const bool f_rs = rs <= 0.0;
    const bool f_score = score < P.min_long_score;
    const bool f_bb = !(reached && change <= P.max_change_pct);
    const bool f_price = !(low < price && price < high);
    const bool f_width = !(P.min_width_pct <= rw && rw <= P.max_width_pct);
    // the first failing check: selects from the last check to the first
    int st = BQ_GL_EMIT;
    st = f_width ? BQ_GL_RANGE_WIDTH : st;
    st = f_price ? BQ_GL_PRICE_OUTSIDE : st;
    st = f_bb ? BQ_GL_BB_EXPANDING : st;
    st = f_score ? BQ_GL_LONG_SCORE_LOW : st;
    st = f_rs ? BQ_GL_RS_NOT_POSITIVE : st;
    st = f_ema ? BQ_GL_BELOW_EMAS : st;
    st = f_trans ? BQ_GL_SYMBOL_TRANSITION : st;
    st = f_micro ? BQ_GL_MICRO_REGIME : st;
    st = f_range ? BQ_GL_NOT_RANGE : st;
    st = f_ctx ? BQ_GL_NO_CONTEXT : st;
    st = f_policy ? BQ_GL_POLICY : st;
    st = (t < begin || t >= len) ? BQ_GL_NO_FRAME : st;
    const int64_t o = orow + t;
    A.status[o] = (uint8_t)st;
    const bool emit = st == BQ_GL_EMIT;
    const bool walked = (emit || st >= BQ_GL_BB_EXPANDING) && reached;   // the method called _bb_stable, which got to :55
    const bool sized = emit || st == BQ_GL_RANGE_WIDTH;
    const double v[BQ_GL_NVALUES] = {walked ? change : qnan(), sized ? rw : qnan(), emit ? buf : qnan(),
                                     emit ? blow : qnan(), emit ? bhigh : qnan()};
#pragma unroll
    for (int c = 0; c < BQ_GL_NVALUES; ++c)
      if (A.val[c]) A.val[c][o] = v[c];   // wave-uniform: a NULL column is skipped
  }
}

}  // namespace bq

extern "C" void bq_grid_ladder_default_params(bq_grid_ladder_params* p) {
  if (!p) return;
  // LadderDeployer's class attributes (strategies/grid/ladder_deployer.py:16-28)
  p->n = 8;
  p->reserved = 0;
  p->max_change_pct = 20.0;
  p->min_width_pct = 1.5;
  p->max_width_pct = 8.0;
  p->min_buffer_pct = 0.5;
  p->max_buffer_pct = 4.0;
  p->atr_multiplier = 1.5;
  p->min_long_score = 0.2;
}

extern "C" int bq_grid_ladder_replay(const double* close, int64_t ld_c, const double* bb_upper, const double* bb_mid,
                                     const double* bb_lower, int64_t ld_bb, const double* bb_high,
                                     const double* bb_mid_arg, const double* bb_low, int64_t ld_bands,
                                     const uint8_t* policy_ok, const uint8_t* ctx_ok, const int8_t* market_regime,
                                     const double* long_regime_score, int64_t ctx_T, const uint8_t* sym_ok,
                                     const uint8_t* sym_micro_regime, const uint8_t* sym_micro_transition,
                                     const uint8_t* sym_above_ema20, const uint8_t* sym_above_ema50,
                                     const double* sym_rs_vs_btc, const double* sym_atr_pct, int64_t ld_sym,
                                     const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S,
                                     int64_t T, const bq_grid_ladder_params* params, uint8_t* status,
                                     double* const* values, int64_t ld_out, void* stream) {
  using namespace bq;
  const bool own_bands = bb_high || bb_mid_arg || bb_low;
  int64_t tiles;
  if (!close || !bb_upper || !bb_mid || !bb_lower || !market_regime || !long_regime_score || !status || S < 0 ||
      T < 0 || ld_c < T || ld_bb < T || ld_out < T || (ld_sym != 0 && ld_sym < T) || (ctx_T != 1 && ctx_T != T) ||
      !candle_tiles(S, T, tiles))
    return BQ_EINVAL;
  if (own_bands && (!bb_high || !bb_mid_arg || !bb_low || ld_bands < T)) return BQ_EINVAL;
  if (sym_ok && (!sym_micro_regime || !sym_micro_transition || !sym_above_ema20 || !sym_above_ema50 ||
                 !sym_rs_vs_btc || !sym_atr_pct))
    return BQ_EINVAL;
  GlArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_grid_ladder_default_params(&A.p);
  const bq_grid_ladder_params& p = A.p;
  if (p.n < 1 || p.n > BQ_BB_STABLE_MAX_N ||
      !all_finite({p.max_change_pct, p.min_width_pct, p.max_width_pct, p.min_buffer_pct, p.max_buffer_pct,
                   p.atr_multiplier, p.min_long_score}))
    return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  A.close = close;
  A.bbu = bb_upper;
  A.bbm = bb_mid;
  A.bbl = bb_lower;
  A.high = own_bands ? bb_high : bb_upper;
  A.mid = own_bands ? bb_mid_arg : bb_mid;
  A.low = own_bands ? bb_low : bb_lower;
  A.ld_bands = own_bands ? ld_bands : ld_bb;
  A.alias = A.high == bb_upper && A.mid == bb_mid && A.low == bb_lower && A.ld_bands == ld_bb;
  A.policy_ok = policy_ok;
  A.ctx_ok = ctx_ok;
  A.regime = market_regime;
  A.score = long_regime_score;
  A.sym_ok = sym_ok;
  A.sym_regime = sym_micro_regime;
  A.sym_transition = sym_micro_transition;
  A.sym_e20 = sym_above_ema20;
  A.sym_e50 = sym_above_ema50;
  A.sym_rs = sym_rs_vs_btc;
  A.sym_atr = sym_atr_pct;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_c = ld_c;
  A.ld_bb = ld_bb;
  A.ld_sym = ld_sym;
  A.ld_out = ld_out;
  A.T = (int)T;
  A.tiles = (int)tiles;
  A.ctx_T = (int)ctx_T;
  A.status = status;
  tile_values(A.val, values);
  hipLaunchKernelGGL(grid_ladder_kernel, dim3((unsigned)(tiles * S)), dim3(GL_NT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
