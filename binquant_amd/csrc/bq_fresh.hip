// Freshness for the panel context build (gfx950): late listings, halts,
// delistings and single missing candles of a [S][T] panel.
//
// The reference keeps, per symbol, the candles it actually received:
// MarketStateStore drops a candle without a close
// (market_regime/market_state_store.py:84) and caps the history at the last
// max_bars of the rest (:28). _build_context(ts) then admits only the symbols
// whose last candle is ts (get_fresh_symbols, :49-54) and gates on the symbols
// ever seen (live_market_context_accumulator.py:96-102, :196-204).
//
// bq_panel_compact turns each row into that history: the present candles
// (finite close) packed to the front in order, plus rank[s][t] = position of
// candle t in the packed row (-1 where absent). The dense feature kernels then
// run on the packed rows unchanged — a window of max_bars packed candles is
// the store's history — and bq_breadth_partial_fresh sums, for every
// timestamp t, the features at [s][rank[s][t]] of the symbols present at t.
#include "bq_device.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

// ---- per-row stream compaction ------------------------------------------------
// One wave per symbol, FC_NW symbols per workgroup; tiles of 256 candles, 4
// consecutive candles per lane (the context pass's tiling). The position of a
// present candle inside the tile comes from four wave ballots (one per lane
// slot): present candles of lower lanes, plus the lane's own earlier slots.
// The running count across tiles is wave-uniform and stays in a register.
// The tile's packed candles go through LDS so that each store instruction
// writes 64 consecutive doubles of the packed row (whole 128-byte lines when
// the running count is a multiple of 16, one contiguous 512-byte run always)
// instead of a lane-strided scatter.
constexpr int FC_NW = 4;
constexpr int FC_K = 4;
constexpr int FC_TT = WAVE * FC_K;

struct CompactArgs {
  const double* in[3];   // high, low, close
  double* out[3];
  int32_t* rank;
  int32_t* n_present;
  int32_t* first_t;
  int32_t* n_invalid;
  int64_t S, ld_in, ld_c, ld_r;
  int T;
};

typedef int fc_int4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void fc_load(const double* __restrict__ row, int tb, int T, bool vec, double (&x)[FC_K]) {
  if (vec && tb + FC_K <= T) {
    const dbl2* p = reinterpret_cast<const dbl2*>(row + tb);
    const dbl2 a = p[0], b = p[1];
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  } else {
#pragma unroll
    for (int k = 0; k < FC_K; ++k) x[k] = (tb + k < T) ? row[tb + k] : qnan();
  }
}

__global__ __launch_bounds__(FC_NW* WAVE) void panel_compact_kernel(const CompactArgs A, int vec_in, int vec_rank) {
  __shared__ double sV[FC_NW][3][FC_TT];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int64_t sym = (int64_t)blockIdx.x * FC_NW + w;
  const bool live = sym < A.S;   // every wave walks all tiles: the barriers below are block-wide
  const int64_t srow = live ? sym : A.S - 1;
  const int T = A.T;
  const double* __restrict__ rH = A.in[0] + srow * A.ld_in;
  const double* __restrict__ rL = A.in[1] + srow * A.ld_in;
  const double* __restrict__ rC = A.in[2] + srow * A.ld_in;
  double* __restrict__ oH = A.out[0] + srow * A.ld_c;
  double* __restrict__ oL = A.out[1] + srow * A.ld_c;
  double* __restrict__ oC = A.out[2] + srow * A.ld_c;
  int32_t* __restrict__ oR = A.rank + srow * A.ld_r;
  const uint64_t below = (1ull << lane) - 1ull;

  int run = 0;        // present candles before this tile (wave-uniform)
  int invalid = 0;    // wave-uniform
  int first = T;      // wave-uniform
  double lastH = 1.0, lastL = 1.0, lastC = 1.0;   // the row's last present candle
  for (int t0 = 0; t0 < T; t0 += FC_TT) {
    const int tb = t0 + FC_K * lane;
    double h[FC_K], l[FC_K], c[FC_K];
    fc_load(rH, tb, T, vec_in != 0, h);
    fc_load(rL, tb, T, vec_in != 0, l);
    fc_load(rC, tb, T, vec_in != 0, c);
    bool pres[FC_K];
    int pos = 0, total = 0, nbad = 0;
    uint64_t m[FC_K];
#pragma unroll
    for (int k = 0; k < FC_K; ++k) {
      const bool in = tb + k < T;
      pres[k] = in && win_ok(c[k]);                        // finite close
      // +-inf close, or a present candle without a finite high / low
      const bool bad = in && ((c[k] == c[k] && !pres[k]) || (pres[k] && !(win_ok(h[k]) && win_ok(l[k]))));
      m[k] = __ballot(pres[k]);
      nbad += __popcll(__ballot(bad));
      pos += __popcll(m[k] & below);
      total += __popcll(m[k]);
    }
    invalid += nbad;
    int rk[FC_K];
#pragma unroll
    for (int k = 0; k < FC_K; ++k) {
      rk[k] = pres[k] ? run + pos : -1;
      if (pres[k]) {
        sV[w][0][pos] = h[k];
        sV[w][1][pos] = l[k];
        sV[w][2][pos] = c[k];
        ++pos;
      }
    }
    if (run == 0 && total > 0) {   // the candle of rank 0 is in this tile
      int ft = T;
#pragma unroll
      for (int k = FC_K - 1; k >= 0; --k)
        if (rk[k] == 0) ft = tb + k;
      // exactly one lane holds it
      const uint64_t who = __ballot(ft != T);
      first = __shfl(ft, __ffsll((unsigned long long)who) - 1, WAVE);
    }
    if (live) {
      if (vec_rank && tb + FC_K <= T) {
        *reinterpret_cast<fc_int4*>(oR + tb) = fc_int4{rk[0], rk[1], rk[2], rk[3]};
      } else {
#pragma unroll
        for (int k = 0; k < FC_K; ++k)
          if (tb + k < T) oR[tb + k] = rk[k];
      }
    }
    __syncthreads();
    if (total > 0) {
#pragma unroll
      for (int j = 0; j < FC_K; ++j) {
        const int e = lane + WAVE * j;
        if (live && e < total) {   // run + total <= T <= ld_c
          oH[run + e] = sV[w][0][e];
          oL[run + e] = sV[w][1][e];
          oC[run + e] = sV[w][2][e];
        }
      }
      lastH = sV[w][0][total - 1];
      lastL = sV[w][1][total - 1];
      lastC = sV[w][2][total - 1];
    }
    run += total;
    __syncthreads();
  }
  if (!live) return;
  // tail [n, T): the last present candle again (1.0 for an empty row) — finite
  // data for the dense feature kernels; nothing gathers from it
  for (int j = run + lane; j < T; j += WAVE) {
    oH[j] = lastH;
    oL[j] = lastL;
    oC[j] = lastC;
  }
  if (lane == 0) {
    A.n_present[sym] = run;
    A.first_t[sym] = first;
    A.n_invalid[sym] = invalid;
  }
}

// ---- breadth partials over the fresh symbols --------------------------------------
// breadth_kernel (bq_market.hip) with a gather: the same constants, the same
// per-wave symbol order and the same combine order, so with every candle
// present (rank[s][t] = t) columns 0-8 are bit-equal to bq_breadth_partial's.
// Neighbouring lanes of a symbol read rank k and k +- 1 except across a gap,
// so the gathers stay near-coalesced. Column BQ_P_RESERVED counts the symbols
// listed at or before t (an integer-valued sum: exact in any order).
constexpr int BF_TW = 64;   // = BR_TW
constexpr int BF_NW = 16;   // = BR_NW

struct FreshArgs {
  const double* c;
  const double* f[BQ_NUM_FEATURES];
  const int32_t* rank;
  const int32_t* first_t;
  int64_t S, ld_c, ld_f, ld_r;
  int T;
  double* partial;
};

// k = rank[s][t], listed = first_t[s] <= t: loaded by the caller one symbol
// ahead, so the gathers of symbol s do not wait behind its own rank load
__device__ __forceinline__ void fresh_accumulate(const FreshArgs& A, int64_t s, int k, bool listed,
                                                 double (&acc)[BQ_NUM_PARTIALS]) {
  acc[BQ_P_RESERVED] += listed ? 1.0 : 0.0;
  if (k < 1 || k >= A.T) return;   // absent at t, or the symbol's first candle (history < 2 bars)
  const double r = A.f[BQ_F_RETURN][s * A.ld_f + k];
  if (r != r) return;
  const double cl = A.c[s * A.ld_c + k];
  acc[BQ_P_COUNT] += 1.0;
  acc[BQ_P_ADV] += r > 0.0 ? 1.0 : 0.0;
  acc[BQ_P_DEC] += r < 0.0 ? 1.0 : 0.0;
  acc[BQ_P_ABOVE20] += cl > A.f[BQ_F_EMA20][s * A.ld_f + k] ? 1.0 : 0.0;
  acc[BQ_P_ABOVE50] += cl > A.f[BQ_F_EMA50][s * A.ld_f + k] ? 1.0 : 0.0;
  acc[BQ_P_SUM_RET] += r;
  acc[BQ_P_SUM_TREND] += A.f[BQ_F_TREND][s * A.ld_f + k];
  acc[BQ_P_SUM_ATR_PCT] += A.f[BQ_F_ATR_PCT][s * A.ld_f + k];
  acc[BQ_P_SUM_BB_WIDTH] += A.f[BQ_F_BB_WIDTH][s * A.ld_f + k];
}

// symbols s0, s0 + step, ... < S at timestamp t, in that order
__device__ __forceinline__ void fresh_walk(const FreshArgs& A, int64_t s0, int step, int t,
                                           double (&acc)[BQ_NUM_PARTIALS]) {
  if (s0 >= A.S) return;
  int k = A.rank[s0 * A.ld_r + t];
  int ft = A.first_t[s0];
  for (int64_t s = s0; s < A.S; s += step) {
    const int64_t sn = s + step < A.S ? s + step : s;   // clamped: the last prefetch re-reads s
    const int kn = A.rank[sn * A.ld_r + t];
    const int fn = A.first_t[sn];
    fresh_accumulate(A, s, k, ft <= t, acc);
    k = kn;
    ft = fn;
  }
}

__global__ __launch_bounds__(BF_TW* BF_NW) void breadth_fresh_kernel(const FreshArgs A) {
  __shared__ double sAcc[BF_NW][BQ_NUM_PARTIALS][BF_TW + 1];
  const int lane = threadIdx.x & (WAVE - 1), u = threadIdx.x / WAVE;
  const int t = blockIdx.x * BF_TW + lane;
  double acc[BQ_NUM_PARTIALS];
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] = 0.0;
  if (t < A.T) fresh_walk(A, u, BF_NW, t, acc);
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) sAcc[u][i][lane] = acc[i];
  __syncthreads();
  if (u == 0 && t < A.T) {
    for (int v = 1; v < BF_NW; ++v)
#pragma unroll
      for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] += sAcc[v][i][lane];
#pragma unroll
    for (int i = 0; i < BQ_NUM_PARTIALS; ++i) A.partial[(int64_t)t * BQ_NUM_PARTIALS + i] = acc[i];
  }
}

// Few timestamps (the live shapes, T <= 256): one workgroup per timestamp,
// thread k sums symbols k, k + BFS_NT, ... in ascending order, then the
// xor-butterflies of breadth_small_kernel (bq_market.hip) combine the
// threads — its order, so the all-present result is bit-equal to it as well.
constexpr int BFS_NT = 1024;   // = BS_NT
constexpr int BFS_MAX_T = 256;   // = BS_MAX_T

__device__ __forceinline__ double fresh_wave_sum(double v, int width) {
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1)
    if (d < width) v += __shfl_xor(v, d, WAVE);
  return v;
}

__global__ __launch_bounds__(BFS_NT) void breadth_fresh_small_kernel(const FreshArgs A) {
  __shared__ double sRed[BQ_NUM_PARTIALS][BFS_NT / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int t = blockIdx.x;
  double acc[BQ_NUM_PARTIALS];
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] = 0.0;
  fresh_walk(A, tid, BFS_NT, t, acc);
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) {
    const double v = fresh_wave_sum(acc[i], WAVE);
    if (lane == 0) sRed[i][w] = v;
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int i = 0; i < BQ_NUM_PARTIALS; ++i) {
      const double v = fresh_wave_sum(lane < BFS_NT / WAVE ? sRed[i][lane] : 0.0, BFS_NT / WAVE);
      if (lane == 0) A.partial[(int64_t)t * BQ_NUM_PARTIALS + i] = v;
    }
  }
}

}  // namespace bq

extern "C" {

int bq_panel_compact(const double* const* hlc, int64_t S, int64_t T, int64_t ld_in, double* const* hlc_out,
                     int64_t ld_c, int32_t* rank, int64_t ld_r, int32_t* n_present, int32_t* first_t,
                     int32_t* n_invalid, void* stream) {
  using namespace bq;
  if (!hlc || !hlc_out || !rank || !n_present || !first_t || !n_invalid || S < 0 || T < 0 || ld_in < T ||
      ld_c < T || ld_r < T || T > (int64_t)0x7fffffff - FC_TT || S > (int64_t)0x7fffffff)
    return BQ_EINVAL;
  for (int i = 0; i < 3; ++i)
    if (!hlc[i] || !hlc_out[i]) return BQ_EINVAL;
  if (S == 0) return BQ_OK;
  CompactArgs A;
  memset(&A, 0, sizeof(A));
  for (int i = 0; i < 3; ++i) {
    A.in[i] = hlc[i];
    A.out[i] = hlc_out[i];
  }
  A.rank = rank;
  A.n_present = n_present;
  A.first_t = first_t;
  A.n_invalid = n_invalid;
  A.S = S;
  A.ld_in = ld_in;
  A.ld_c = ld_c;
  A.ld_r = ld_r;
  A.T = (int)T;
  auto aligned = [](const void* p) { return (((uintptr_t)p) & 15u) == 0; };
  const int vin = (ld_in % 2) == 0 && aligned(hlc[0]) && aligned(hlc[1]) && aligned(hlc[2]);
  const int vrank = (ld_r % 4) == 0 && aligned(rank);
  const unsigned blocks = (unsigned)((S + FC_NW - 1) / FC_NW);
  hipLaunchKernelGGL(panel_compact_kernel, dim3(blocks), dim3(FC_NW * WAVE), 0, (hipStream_t)stream, A, vin, vrank);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

int bq_breadth_partial_fresh(const double* close_c, const double* const* feat_c, const int32_t* rank,
                             const int32_t* first_t, int64_t S, int64_t T, int64_t ld_c, int64_t ld_f,
                             int64_t ld_r, double* partial, void* stream) {
  using namespace bq;
  if (!close_c || !feat_c || !rank || !first_t || !partial || S < 0 || T < 0 || ld_c < T || ld_f < T ||
      ld_r < T || T > 0x7fffffff)
    return BQ_EINVAL;
  for (int i = 0; i < BQ_NUM_FEATURES; ++i)
    if (!feat_c[i]) return BQ_EINVAL;
  if (T == 0) return BQ_OK;
  FreshArgs A;
  A.c = close_c;
  for (int i = 0; i < BQ_NUM_FEATURES; ++i) A.f[i] = feat_c[i];
  A.rank = rank;
  A.first_t = first_t;
  A.S = S;
  A.ld_c = ld_c;
  A.ld_f = ld_f;
  A.ld_r = ld_r;
  A.T = (int)T;
  A.partial = partial;
  if (T <= BFS_MAX_T) {
    hipLaunchKernelGGL(breadth_fresh_small_kernel, dim3((unsigned)T), dim3(BFS_NT), 0, (hipStream_t)stream, A);
  } else {
    const unsigned blocks = (unsigned)((T + BF_TW - 1) / BF_TW);
    hipLaunchKernelGGL(breadth_fresh_kernel, dim3(blocks), dim3(BF_TW * BF_NW), 0, (hipStream_t)stream, A);
  }
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // extern "C"
