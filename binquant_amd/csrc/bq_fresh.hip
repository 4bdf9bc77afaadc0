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
// the store's history — and bq_breadth_partial_fresh (bq_breadth.hip) sums,
// for every timestamp t, the features at [s][rank[s][t]] of the symbols
// present at t.
#include "bq_context.h"
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
constexpr int FC_K = CTX_K;
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
    load4<dbl2, true>(rH, tb, T, vec_in != 0, h);
    load4<dbl2, true>(rL, tb, T, vec_in != 0, l);
    load4<dbl2, true>(rC, tb, T, vec_in != 0, c);
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
  const int vin = vec_rows(hlc, 3, ld_in);
  const int vrank = (ld_r % 4) == 0 && aligned16(rank);
  const unsigned blocks = (unsigned)((S + FC_NW - 1) / FC_NW);
  hipLaunchKernelGGL(panel_compact_kernel, dim3(blocks), dim3(FC_NW * WAVE), 0, (hipStream_t)stream, A, vin, vrank);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}

}  // extern "C"
