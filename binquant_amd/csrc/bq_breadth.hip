// Breadth partials for gfx950: the per-timestamp counts and sums of
// _build_context (market_regime/live_market_context_accumulator.py:135-163)
// over the symbols of a shard, in a fixed order.
//
// bq_breadth_partial (dense) sums the features at [s][t] of every symbol.
// bq_breadth_partial_fresh sums, over a panel compacted by bq_panel_compact
// (bq_fresh.hip), the features at [s][rank[s][t]] of the symbols present at t
// (get_fresh_symbols, market_regime/market_state_store.py:49-54), and counts in
// column BQ_P_RESERVED the symbols listed at or before t (an integer-valued
// sum: exact in any order).
//
// Both are the same two kernels, templated on FRESH: one symbol walk, one
// accumulate block, one combine. With every candle present (rank[s][t] = t)
// columns 0-8 of the fresh result are therefore bit-equal to the dense one's,
// at every T. No atomics: bitwise reproducible run to run.
#include "bq_device.h"
#include "binquant_amd.h"

namespace bq {

struct BreadthArgs {
  const double* c;
  const double* f[BQ_NUM_FEATURES];
  const int32_t* rank;      // FRESH only: [S][ld_r]
  const int32_t* first_t;   // FRESH only: [S]
  int64_t S, ld_c, ld_f, ld_r;
  int T;
  double* partial;
};

// symbol s's features at column k into the nine sums. ARGS is how the walk
// hands A over, BreadthArgs or const BreadthArgs&: the source is one, but the
// compiler's loop differs with it. By value the dense walk advances scalar row
// pointers (46 VGPRs); by reference it forms the seven addresses per symbol on
// the VALU (58 VGPRs, +1 % at 12 500 x 2 000), while the fresh walk, whose
// addresses follow the gathered k anyway, is the leaner by reference (52
// against 60 VGPRs, by value +0.7 %; profiles/context_refactor_ab.txt).
template <typename ARGS>
__device__ __forceinline__ void breadth_add(ARGS A, int64_t s, int k, double (&acc)[BQ_NUM_PARTIALS]) {
  const double r = A.f[BQ_F_RETURN][s * A.ld_f + k];
  if (r != r) return;   // no features there (history < 2 bars)
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
template <bool FRESH>
__device__ __forceinline__ void breadth_walk(const BreadthArgs& A, int64_t s0, int step, int t,
                                             double (&acc)[BQ_NUM_PARTIALS]) {
  if constexpr (!FRESH) {
    for (int64_t s = s0; s < A.S; s += step) breadth_add<BreadthArgs>(A, s, t, acc);
  } else {
    // k = rank[s][t] and first_t[s] are loaded one symbol ahead, so the gathers
    // of symbol s do not wait behind its own rank load. Neighbouring lanes of a
    // symbol read rank k and k +- 1 except across a gap: near-coalesced gathers.
    if (s0 >= A.S) return;
    int k = A.rank[s0 * A.ld_r + t];
    int ft = A.first_t[s0];
    for (int64_t s = s0; s < A.S; s += step) {
      const int64_t sn = s + step < A.S ? s + step : s;   // clamped: the last prefetch re-reads s
      const int kn = A.rank[sn * A.ld_r + t];
      const int fn = A.first_t[sn];
      acc[BQ_P_RESERVED] += ft <= t ? 1.0 : 0.0;   // listed at or before t
      // absent at t (-1), or the symbol's first candle (history < 2 bars)
      if (k >= 1 && k < A.T) breadth_add<const BreadthArgs&>(A, s, k, acc);
      k = kn;
      ft = fn;
    }
  }
}

// One workgroup of BR_NW waves owns BR_TW consecutive timestamps; wave u sums
// symbols s = u, u + BR_NW, ... in ascending order, lane = timestamp. The wave
// partials are then combined in wave order: a fixed, placement-independent
// reduction order.
constexpr int BR_TW = 64;
constexpr int BR_NW = 16;

template <bool FRESH>
__global__ __launch_bounds__(BR_TW * BR_NW) void breadth_kernel(const BreadthArgs A) {
  __shared__ double sAcc[BR_NW][BQ_NUM_PARTIALS][BR_TW + 1];
  const int lane = threadIdx.x & (WAVE - 1), u = threadIdx.x / WAVE;
  const int t = blockIdx.x * BR_TW + lane;
  double acc[BQ_NUM_PARTIALS];
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] = 0.0;
  if (t < A.T) breadth_walk<FRESH>(A, u, BR_NW, t, acc);
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) sAcc[u][i][lane] = acc[i];
  __syncthreads();
  if (u == 0 && t < A.T) {
    for (int v = 1; v < BR_NW; ++v)
#pragma unroll
      for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] += sAcc[v][i][lane];
#pragma unroll
    for (int i = 0; i < BQ_NUM_PARTIALS; ++i) A.partial[(int64_t)t * BQ_NUM_PARTIALS + i] = acc[i];
  }
}

// Few timestamps (the live tick: T = 1). The kernel above gives one lane per
// timestamp, so at T = 1 each of its 16 waves walks S / 16 symbols with one
// active lane (≈0.5 ms at S = 10k). Here a workgroup of BS_NT threads owns one
// timestamp: thread k sums symbols k, k + BS_NT, ... in ascending order, then
// xor-butterflies over the wave and over the waves combine the threads. Again a
// fixed, placement-independent order.
constexpr int BS_NT = 1024;
constexpr int BS_MAX_T = 256;

__device__ __forceinline__ double wave_sum(double v, int width) {
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1)
    if (d < width) v += __shfl_xor(v, d, WAVE);
  return v;
}

template <bool FRESH>
__global__ __launch_bounds__(BS_NT) void breadth_small_kernel(const BreadthArgs A) {
  __shared__ double sRed[BQ_NUM_PARTIALS][BS_NT / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int t = blockIdx.x;
  double acc[BQ_NUM_PARTIALS];
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) acc[i] = 0.0;
  breadth_walk<FRESH>(A, tid, BS_NT, t, acc);
#pragma unroll
  for (int i = 0; i < BQ_NUM_PARTIALS; ++i) {
    const double v = wave_sum(acc[i], WAVE);
    if (lane == 0) sRed[i][w] = v;
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int i = 0; i < BQ_NUM_PARTIALS; ++i) {
      const double v = wave_sum(lane < BS_NT / WAVE ? sRed[i][lane] : 0.0, BS_NT / WAVE);
      if (lane == 0) A.partial[(int64_t)t * BQ_NUM_PARTIALS + i] = v;
    }
  }
}

// checks the arguments, then the small kernel up to BS_MAX_T timestamps, the
// big one beyond; rank / first_t / ld_r are read with FRESH only
template <bool FRESH>
static int breadth_partial(const double* close, const double* const* feat, const int32_t* rank,
                           const int32_t* first_t, int64_t S, int64_t T, int64_t ld_c, int64_t ld_f, int64_t ld_r,
                           double* partial, hipStream_t st) {
  if (!close || !feat || !partial || S < 0 || T < 0 || ld_c < T || ld_f < T || T > 0x7fffffff) return BQ_EINVAL;
  if (FRESH && (!rank || !first_t || ld_r < T)) return BQ_EINVAL;
  for (int i = 0; i < BQ_NUM_FEATURES; ++i)
    if (!feat[i]) return BQ_EINVAL;
  if (T == 0) return BQ_OK;
  BreadthArgs A;
  A.c = close;
  for (int i = 0; i < BQ_NUM_FEATURES; ++i) A.f[i] = feat[i];
  A.rank = rank;
  A.first_t = first_t;
  A.S = S;
  A.ld_c = ld_c;
  A.ld_f = ld_f;
  A.ld_r = ld_r;
  A.T = (int)T;
  A.partial = partial;
  if (T <= BS_MAX_T) {
    hipLaunchKernelGGL(breadth_small_kernel<FRESH>, dim3((unsigned)T), dim3(BS_NT), 0, st, A);
  } else {
    const unsigned blocks = (unsigned)((T + BR_TW - 1) / BR_TW);
    hipLaunchKernelGGL(breadth_kernel<FRESH>, dim3(blocks), dim3(BR_TW * BR_NW), 0, st, A);
  }
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // namespace bq

extern "C" {

int bq_breadth_partial(const double* close, const double* const* feat, int64_t S, int64_t T,
                       int64_t ld_close, int64_t ld_feat, double* partial, void* stream) {
  return bq::breadth_partial<false>(close, feat, nullptr, nullptr, S, T, ld_close, ld_feat, 0, partial,
                                    (hipStream_t)stream);
}

int bq_breadth_partial_fresh(const double* close_c, const double* const* feat_c, const int32_t* rank,
                             const int32_t* first_t, int64_t S, int64_t T, int64_t ld_c, int64_t ld_f,
                             int64_t ld_r, double* partial, void* stream) {
  return bq::breadth_partial<true>(close_c, feat_c, rank, first_t, S, T, ld_c, ld_f, ld_r, partial,
                                   (hipStream_t)stream);
}

}  // extern "C"
