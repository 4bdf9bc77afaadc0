// LiquidationSweepPump's candidate gate and the cohort's winner on a [S][T]
// panel (gfx950): everything of signal() between compute_pump_score and the
// portfolio selector (strategies/liquidation_sweep_pump.py:302-343) — the
// frame-length gate (:314), _is_candidate on df.iloc[-2] (:271-300),
// score_threshold <= 0 (:331), rank_score = pump_score / score_threshold
// (:333), the routing verdict (:343) — and, per candle column, the candidate
// LiquidationSweepPortfolioSelector._dispatch_winner would dispatch (:78-81):
// the largest (rank_score, symbol). Column u is the TRIGGER candle: the
// decision taken on df.iloc[-2] at the message whose frame is
// df.iloc[first : u + 2].
//
// The winner is an arg-max DOWN a column (over symbols); the panel is
// row-major, so two mappings, chosen by the width of [t_lo, t_hi):
//
//   wide (>= SW_SWITCH columns, the panel replay): a lane owns a candle
//     column, a wave reads 64 consecutive candles of one row as one 512-byte
//     segment per input column; a 256-thread workgroup covers 256 candles x
//     SW_ROWS rows and walks its rows with each lane's running best
//     (key, rank, row) in registers — no cross-lane step at all. The 13 + 2
//     loads of row r + 1 are issued before row r is tested (the gate has no
//     arithmetic to hide a load behind). Status bytes and rank_score go out as
//     the same coalesced segments; the chunk's per-column best goes to the
//     workspace.
//   narrow (< SW_SWITCH columns, the cohort's one column): a lane owns a row
//     and loads the strided cell; the arg-max is a wave butterfly, the four
//     waves meet in LDS, the workgroup's best goes to the workspace. Lanes past
//     S and rows that are not candidates carry the "none" key 0.
//
// Both end in sweep_merge_kernel: per column, sixteen waves fold the partials
// (row chunks or workgroups) and meet in LDS. Every partial the merge reads was
// written by the same call, so the workspace needs no initialisation, and the
// order (key, rank, row) is total, so the result does not depend on the launch
// geometry. Scores compare through order_key (bq_device.h); a candidate's score
// is >= 1 or +inf, never NaN, so key 0 is free to mean "no candidate".
#include "bq_device.h"
#include "binquant_amd.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace bq {

constexpr int SW_NT = 256;      // threads: candles per wide tile, rows per narrow workgroup
constexpr int SW_ROWS = 64;     // rows per wide chunk: 12.5k x 2k -> 196 chunks x 8 tiles = 1568 workgroups, ~6 per CU
constexpr int SW_SWITCH = 64;   // narrower ranges cannot fill a wave's 512-byte segment: lane = row
constexpr int SW_MG = 16;       // waves of a merge workgroup: slices of the partials per column
constexpr int SW_NONE_RANK = -0x7fffffff - 1;

struct SwArgs {
  const double* col[BQ_SW_NCOLS];
  const uint8_t *cross, *route;
  const int64_t *lens, *first;
  const int32_t* srank;
  int64_t ld_in, ld_b, ld_r, ld_out;
  int S, T, t_lo, t_hi;
  bq_sweep_params p;
  uint8_t* status;
  double* rank;
  uint64_t* pkey;   // partials [parts][ncol]: the best key (0: none), its rank and row
  int32_t *prank, *prow;
  int ncol;
};

struct SwCell {
  double v[BQ_SW_NCOLS];
  uint8_t cross, route;
};

// ROUTE false: no route mask, every cell allowed. A compile-time choice: the
// loads of a row stay one straight line (a branch around one of them would make
// the wait for a row's cell drain the next row's loads too), and the walk is
// bound by its memory instructions, so a mask that is not there is not loaded.
template <bool ROUTE>
__device__ __forceinline__ void sw_load(const SwArgs& A, int64_t row, int u, SwCell& c) {
  const int64_t i = row * A.ld_in + u;
#pragma unroll
  for (int k = 0; k < BQ_SW_NCOLS; ++k) c.v[k] = A.col[k][i];
  c.cross = A.cross[row * A.ld_b + u];
  c.route = ROUTE ? A.route[row * A.ld_r + u] : (uint8_t)1;
}

// the first failing check in signal()'s order; every compare in the method's
// direction (a NaN fails it; after NOT_FINITE none is left)
__device__ __forceinline__ int sw_status(const SwCell& c, int u, int64_t first, int64_t len,
                                         const bq_sweep_params& P) {
  const double thr = c.v[1], matr = c.v[2], close = c.v[3], ph = c.v[4], cl = c.v[5], rv = c.v[6],
               vthr = c.v[7], trend = c.v[8], ema20 = c.v[9], rs = c.v[10], bm = c.v[11], bt = c.v[12];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < BQ_SW_NCOLS; ++k) fin &= win_ok(c.v[k]);
  int st = BQ_SW_CANDIDATE;
  st = c.route ? st : BQ_SW_ROUTE_REFUSED;                                   // :343
  st = thr <= 0.0 ? BQ_SW_THRESHOLD_NONPOSITIVE : st;                        // :331
  st = bt > 0.0 ? st : BQ_SW_BTC_TREND;                                      // :299
  st = bm > 0.0 ? st : BQ_SW_BTC_MOMENTUM;                                   // :298
  st = rs > 0.0 ? st : BQ_SW_RELATIVE_STRENGTH;                              // :297
  st = close > ema20 ? st : BQ_SW_BELOW_EMA20;                               // :296
  st = trend > 0.0 ? st : BQ_SW_TREND;                                       // :295
  st = rv >= vthr ? st : BQ_SW_VOLUME;                                       // :294
  st = cl >= P.min_close_location ? st : BQ_SW_CLOSE_LOCATION;               // :293
  st = close > ph ? st : BQ_SW_NOT_ABOVE_PRIOR_HIGH;                         // :292
  st = ((P.min_momentum_atr <= matr) & (matr <= P.max_momentum_atr)) ? st : BQ_SW_MOMENTUM_ATR;   // :291
  st = c.cross ? st : BQ_SW_NO_CROSS;                                        // :290
  st = fin ? st : BQ_SW_NOT_FINITE;                                          // :287
  st = (int64_t)u + 2 - first >= (int64_t)P.min_frame ? st : BQ_SW_SHORT_FRAME;   // :314
  st = (((int64_t)u + 1 >= len) | ((int64_t)u < first)) ? BQ_SW_NO_FRAME : st;
  return st;
}

// (key, rank, row) of a beats b: _dispatch_winner's max(key=(rank_score,
// symbol)), then the larger row among equal ranks
__device__ __forceinline__ bool sw_better(uint64_t ka, int ra, int wa, uint64_t kb, int rb, int wb) {
  return ka > kb || (ka == kb && (ra > rb || (ra == rb && wa > wb)));
}

template <bool ROUTE>
__global__ __launch_bounds__(SW_NT) void sweep_wide_kernel(const SwArgs A, int ntiles) {
  // the chunk's row scalars, through LDS: inside the walk they would be vector
  // loads that the wait for a row's cell could not tell from the next row's
  __shared__ int64_t sFirst[SW_ROWS], sLen[SW_ROWS];
  __shared__ int sRank[SW_ROWS];
  const int tile = (int)(blockIdx.x % (unsigned)ntiles), chunk = (int)(blockIdx.x / (unsigned)ntiles);
  const int r0 = chunk * SW_ROWS, r1 = min(r0 + SW_ROWS, A.S);   // chunk < ceil(S / SW_ROWS): r0 < S
  if ((int)threadIdx.x < r1 - r0) {
    const int r = r0 + (int)threadIdx.x;
    sFirst[threadIdx.x] = A.first ? A.first[r] : 0;
    sLen[threadIdx.x] = A.lens ? A.lens[r] : (int64_t)A.T;
    sRank[threadIdx.x] = A.srank ? A.srank[r] : r;
  }
  __syncthreads();
  const int j = tile * SW_NT + (int)threadIdx.x;   // column of the range
  if (j >= A.ncol) return;                         // no barrier below
  const int u = A.t_lo + j;
  uint64_t bkey = 0;
  int brank = SW_NONE_RANK, brow = -1;
  auto test = [&](const SwCell& c, int r) {
    const int st = sw_status(c, u, sFirst[r - r0], sLen[r - r0], A.p);
    const int64_t o = (int64_t)r * A.ld_out + u;
    A.status[o] = (uint8_t)st;
    double score = qnan();
    if (st == BQ_SW_CANDIDATE) {
      score = c.v[0] / c.v[1];   // one correctly rounded divide (:333)
      const uint64_t key = order_key(score);
      const int rk = sRank[r - r0];
      if (sw_better(key, rk, r, bkey, brank, brow)) {
        bkey = key;
        brank = rk;
        brow = r;
      }
    }
    if (A.rank) A.rank[o] = score;
  };
  // Two cell buffers that swap roles (a copy would have to wait for the
  // loads): row r + 1 is in flight while row r is tested. Past the chunk's end
  // the last row is loaded again rather than branching around the loads.
  SwCell even, odd;
  sw_load<ROUTE>(A, r0, u, even);
  for (int r = r0; r < r1; r += 2) {
    sw_load<ROUTE>(A, min(r + 1, r1 - 1), u, odd);
    test(even, r);
    sw_load<ROUTE>(A, min(r + 2, r1 - 1), u, even);
    if (r + 1 < r1) test(odd, r + 1);
  }
  const int64_t pi = (int64_t)chunk * A.ncol + j;
  A.pkey[pi] = bkey;
  A.prank[pi] = brank;
  A.prow[pi] = brow;
}

template <bool ROUTE>
__global__ __launch_bounds__(SW_NT) void sweep_narrow_kernel(const SwArgs A) {
  __shared__ uint64_t sK[SW_NT / WAVE];
  __shared__ int sR[SW_NT / WAVE], sW[SW_NT / WAVE];
  const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int64_t r64 = (int64_t)blockIdx.x * SW_NT + tid;
  const bool live = r64 < (int64_t)A.S;
  const int r = live ? (int)r64 : 0;
  const int64_t first = live && A.first ? A.first[r] : 0, len = live && A.lens ? A.lens[r] : (int64_t)A.T;
  const int rk = live && A.srank ? A.srank[r] : r;
  for (int u = A.t_lo; u < A.t_hi; ++u) {   // the same trip count in every thread: the barriers are uniform
    uint64_t key = 0;   // a lane past S, or a row that is no candidate: "none"
    int rank = SW_NONE_RANK, row = -1;
    if (live) {
      SwCell c;
      sw_load<ROUTE>(A, r, u, c);
      const int st = sw_status(c, u, first, len, A.p);
      const int64_t o = (int64_t)r * A.ld_out + u;
      A.status[o] = (uint8_t)st;
      double score = qnan();
      if (st == BQ_SW_CANDIDATE) {
        score = c.v[0] / c.v[1];
        key = order_key(score);
        rank = rk;
        row = r;
      }
      if (A.rank) A.rank[o] = score;
    }
#pragma unroll
    for (int m = WAVE / 2; m > 0; m >>= 1) {
      const uint64_t k2 = __shfl_xor(key, m, WAVE);
      const int r2 = __shfl_xor(rank, m, WAVE), w2 = __shfl_xor(row, m, WAVE);
      if (sw_better(k2, r2, w2, key, rank, row)) {
        key = k2;
        rank = r2;
        row = w2;
      }
    }
    if (lane == 0) {
      sK[wave] = key;
      sR[wave] = rank;
      sW[wave] = row;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < SW_NT / WAVE; ++w)
        if (sw_better(sK[w], sR[w], sW[w], key, rank, row)) {
          key = sK[w];
          rank = sR[w];
          row = sW[w];
        }
      const int64_t pi = (int64_t)blockIdx.x * A.ncol + (u - A.t_lo);
      A.pkey[pi] = key;
      A.prank[pi] = rank;
      A.prow[pi] = row;
    }
    __syncthreads();   // the next column rewrites the LDS slots
  }
}

// 64 columns per workgroup, SW_MG waves: wave g folds the partials g, g +
// SW_MG, ... of its lane's column, the waves meet in LDS (a lane alone would
// walk all the row chunks of a tall panel one dependent step at a time)
__global__ __launch_bounds__(WAVE * SW_MG) void sweep_merge_kernel(const uint64_t* __restrict__ pkey,
                                                                   const int32_t* __restrict__ prank,
                                                                   const int32_t* __restrict__ prow, int parts,
                                                                   int ncol, int t_lo, int64_t* __restrict__ winner,
                                                                   double* __restrict__ winner_score) {
  __shared__ uint64_t sK[SW_MG][WAVE];
  __shared__ int sR[SW_MG][WAVE], sW[SW_MG][WAVE];
  const int lane = (int)threadIdx.x & (WAVE - 1), g = (int)threadIdx.x / WAVE;
  const int j = (int)blockIdx.x * WAVE + lane;
  uint64_t bkey = 0;
  int brank = SW_NONE_RANK, brow = -1;
  if (j < ncol) {
#pragma unroll 4
    for (int p = g; p < parts; p += SW_MG) {
      const int64_t pi = (int64_t)p * ncol + j;
      const uint64_t k = pkey[pi];
      const int rk = prank[pi], w = prow[pi];
      if (sw_better(k, rk, w, bkey, brank, brow)) {
        bkey = k;
        brank = rk;
        brow = w;
      }
    }
  }
  sK[g][lane] = bkey;
  sR[g][lane] = brank;
  sW[g][lane] = brow;
  __syncthreads();
  if (g != 0 || j >= ncol) return;
#pragma unroll
  for (int q = 1; q < SW_MG; ++q)
    if (sw_better(sK[q][lane], sR[q][lane], sW[q][lane], bkey, brank, brow)) {
      bkey = sK[q][lane];
      brank = sR[q][lane];
      brow = sW[q][lane];
    }
  winner[t_lo + j] = (int64_t)brow;   // -1: the column has no candidate
  if (winner_score) winner_score[t_lo + j] = bkey ? key_value(bkey) : qnan();
}

}  // namespace bq

namespace {
// partials of either mapping: parts x ncol entries of 8 + 4 + 4 bytes
int64_t sw_parts(int64_t S, int64_t width) {
  return width >= bq::SW_SWITCH ? (S + bq::SW_ROWS - 1) / bq::SW_ROWS : (S + bq::SW_NT - 1) / bq::SW_NT;
}
}  // namespace

extern "C" void bq_sweep_default_params(bq_sweep_params* p) {
  if (!p) return;
  // LiquidationSweepPump's class attributes (:94-101)
  p->min_momentum_atr = 0.75;
  p->max_momentum_atr = 3.0;
  p->min_close_location = 0.70;
  p->min_frame = 48 + 6 + 2;   // SCORE_LOOKBACK + COMPRESSION_BARS + 2 (:314)
  p->reserved = 0;
}

extern "C" int64_t bq_sweep_select_workspace(int64_t S, int64_t T) {
  if (S <= 0 || T <= 0) return 0;
  // the wide mapping's row chunks at the full width bound every range of either mapping
  return 16 * ((S + bq::SW_ROWS - 1) / bq::SW_ROWS) * T;
}

extern "C" int bq_sweep_select(const double* const* cols, int64_t ld_in, const uint8_t* score_cross, int64_t ld_b,
                               const uint8_t* route_ok, int64_t ld_r, const int64_t* lens, const int64_t* first_t,
                               const int32_t* symbol_rank, int64_t S, int64_t T, int64_t t_lo, int64_t t_hi,
                               const bq_sweep_params* params, uint8_t* status, double* rank_score, int64_t ld_out,
                               int64_t* winner, double* winner_score, void* workspace, void* stream) {
  using namespace bq;
  if (!cols || !score_cross || !status || !winner || !workspace || S < 0 || T < 0 || S > 0x7fffffff ||
      T > 0x7fffffff || ld_in < T || ld_b < T || ld_out < T || (route_ok && ld_r < T) || t_lo < 0 || t_hi > T ||
      t_lo > t_hi || ((uintptr_t)workspace & 7u))
    return BQ_EINVAL;
  for (int k = 0; k < BQ_SW_NCOLS; ++k)
    if (!cols[k]) return BQ_EINVAL;
  SwArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_sweep_default_params(&A.p);
  if (!std::isfinite(A.p.min_momentum_atr) || !std::isfinite(A.p.max_momentum_atr) ||
      !std::isfinite(A.p.min_close_location) || A.p.min_momentum_atr > A.p.max_momentum_atr)
    return BQ_EINVAL;
  if (S == 0 || T == 0 || t_lo == t_hi) return BQ_OK;
  const int64_t width = t_hi - t_lo, parts = sw_parts(S, width);
  const bool wide = width >= SW_SWITCH;
  const int64_t ntiles = (width + SW_NT - 1) / SW_NT;
  if (wide && parts * ntiles > 0x7fffffff) return BQ_EINVAL;   // one grid dimension
  for (int k = 0; k < BQ_SW_NCOLS; ++k) A.col[k] = cols[k];
  A.cross = score_cross;
  A.route = route_ok;
  A.lens = lens;
  A.first = first_t;
  A.srank = symbol_rank;
  A.ld_in = ld_in;
  A.ld_b = ld_b;
  A.ld_r = ld_r;
  A.ld_out = ld_out;
  A.S = (int)S;
  A.T = (int)T;
  A.t_lo = (int)t_lo;
  A.t_hi = (int)t_hi;
  A.status = status;
  A.rank = rank_score;
  A.ncol = (int)width;
  A.pkey = static_cast<uint64_t*>(workspace);
  A.prank = reinterpret_cast<int32_t*>(A.pkey + parts * width);
  A.prow = A.prank + parts * width;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(wide ? (unsigned)(parts * ntiles) : (unsigned)parts);
  if (wide && route_ok) hipLaunchKernelGGL(sweep_wide_kernel<true>, grid, dim3(SW_NT), 0, st, A, (int)ntiles);
  else if (wide) hipLaunchKernelGGL(sweep_wide_kernel<false>, grid, dim3(SW_NT), 0, st, A, (int)ntiles);
  else if (route_ok) hipLaunchKernelGGL(sweep_narrow_kernel<true>, grid, dim3(SW_NT), 0, st, A);
  else hipLaunchKernelGGL(sweep_narrow_kernel<false>, grid, dim3(SW_NT), 0, st, A);
  hipLaunchKernelGGL(sweep_merge_kernel, dim3((unsigned)((width + WAVE - 1) / WAVE)), dim3(WAVE * SW_MG), 0, st, A.pkey,
                     A.prank, A.prow, (int)parts, (int)width, (int)t_lo, winner, winner_score);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
