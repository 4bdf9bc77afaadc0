// RelativeStrengthReversalRange.signal() replayed over a [S][T] panel of 15m
// frames (gfx950; strategies/relative_strength_reversal_range.py:75-101 with
// regime_routing :56-73): the frame gate, the route gate and the 24 h volume
// floor. Column t of row s = the method on the message whose frame is
// df.iloc[first_t[s]:t + 1]; the method keeps no state (the rule table:
// include/binquant_amd.h).
//
// rs_reversal_kernel<EPL>: the wave-per-row replay mapping (bq_replay.h).
//   1. the gates come first: the frame length, the context of the candle's
//      time (present, its regime, average_return) and the symbol's snapshot
//      entry (present, relative_strength_vs_btc), 26 B a candle at most. A
//      ballot of the lanes that pass them all decides the step: with none the
//      wave writes its codes and moves on, no sort and no further load. The
//      route lets few candles through (RANGE, a weak market and a leader), so
//      most steps of a backtest end here.
//   2. otherwise the floor, recent_volume.quantile(q) = Series.quantile =
//      np.percentile(method="linear") over the non-NaN rows of the window:
//      the windows of the step's 64 candles lie in the union
//      volume[t0 - window + 1 .. t0 + 63], window + 63 <= 64 * EPL slots. The
//      wave loads the union (slot u = lane * EPL + e: the two / four nearest
//      partners of the network stay in the lane's registers), sorts it once,
//      a bitonic network over exact order-preserving u64 keys with NaN last
//      and +-inf as values, the union slot as payload, and each reaching lane
//      picks its two ranks among the members of its own window: slot u's
//      one-hot mask of its sorted index, the wave's XOR prefix X(u) over the
//      slots, the window's members in sorted order = the bits of
//      X(lane + window - 1) ^ X(lane - 1), the rank by select_bit. n, the
//      window's non-NaN count, is a difference of prefix counts. The keys,
//      lane moves, scan and selection are bq_rolling.hip's tile rank
//      kernel's (bq_sortsel.h); the values do not pass through win_val.
//   3. the interpolation is numpy's two-sided lerp as bq_select.hip writes it
//      (no FMA: -ffp-contract=off), applied also where the fraction is 0: a
//      finite rank beside an infinite one gives NaN, and the method emits.
//   4. a sorted union of 256 slots holds the windows of two steps where
//      window <= 129: a sorting step then picks the next step's floors too
//      (for every lane: a pick costs the wave the same whatever its lanes'
//      gates say) and hands them on in a register; the next step sorts nothing
//      and loads nothing more. The prefix masks are kept only for the slots a
//      step's window ends read, written again for the second pick: 4 KiB a
//      wave, not 8.
//   Waves of a workgroup walk rows of different lengths: each wave's LDS is
//   its own, ordered by wavefront fences; there is no workgroup barrier.
//   No state of the method is carried from step to step, so the steps before
//   from_t's are not read at all.
//   17 B in (volume, features_ok, relative strength) and 1 + 8 B out per
//   candle, the context [T] from cache; no atomics, no scratch.
//   Resource usage (gfx950 cross-compile, -O3): <4> 92 VGPRs, 80 SGPRs, 5 waves
//   / SIMD (asked for: 101 VGPRs and 4 waves otherwise), LDS 27 680 B a
//   workgroup (4 waves x 6 920 B); <2> 57 VGPRs, 66 SGPRs, 8 waves / SIMD, LDS
//   13 856 B. No spills, scratch 0 in both.
#include "bq_replay.h"
#include "bq_sortsel.h"
#include "binquant_amd.h"

#include <string.h>

namespace bq {

struct RsrArgs {
  const double *volume, *avg_ret, *rs;
  const uint8_t *ctx_ok, *feat_ok;
  const int8_t* regime;
  const int64_t *lens, *first, *from;
  int64_t ld_v, ld_sym, ld_out, S;
  int T, ctx_T, omask;
  bq_rs_reversal_params p;
  uint8_t* status;
  double* val[BQ_RSR_NVALUES];
};

struct RsrStep {
  double v, ar, rs;   // volume[t], the context's average_return, the symbol's relative_strength_vs_btc
  int mk;             // the context's market regime (negative: None)
  bool cok, fok;      // a context is present, it has features for the symbol
};

// one wave's share of LDS: N = 64 * EPL sorted slots
template <int EPL>
struct RsrLds {
  static constexpr int N = WAVE * EPL, NWORD = N / 32;
  unsigned long long key[N];   // the sorted keys
  // XOR prefix of the one-hot masks through union slot u, kept for the slots the ends of a step's windows read
  // (off: 0 for the sorted step, 64 for the one after it):
  unsigned Xlo[WAVE][NWORD];   // u = off - 1 .. off + 62 (just before the window of lane u - off + 1)
  unsigned Xhi[WAVE][NWORD];   // u = off + window - 1 .. off + window + 62 (the last slot of lane u - off - window + 1's)
  unsigned short cnt[N + 2];   // non-NaN values before union slot u
  unsigned char idx[N];        // union slot -> sorted index
};

// what a wave wrote to its LDS is visible to its other lanes, and reads issued before are done
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a sorted union serves the step after its own too where both steps' windows fit its slots (and the count table)
template <int EPL>
__device__ __forceinline__ bool rsr_pair(int W) {
  return W <= WAVE * EPL - (2 * WAVE - 1);
}

// The volume floors of candles t0 .. t0 + 63, and with `pair` those of t0 + 64 .. t0 + 127 into `next` (every lane
// executes it; a floor is used by a reaching lane, whose window volume[t - W + 1 .. t] lies inside the frame):
// union slot u is candle t0 - W + 1 + u.
template <int EPL>
__device__ __forceinline__ double rsr_floor(RsrLds<EPL>& L, const double* __restrict__ vol, int t0, int first, int len,
                                            int W, double q, int lane, bool pair, double& next) {
  constexpr int N = RsrLds<EPL>::N, NWORD = RsrLds<EPL>::NWORD;
  // the network's lane predicates are formed here, step by step: as loop invariants of the row walk they would be
  // held as SGPR pairs, one per stage, and spill
  asm volatile("" : "+v"(lane));
  const int ubase = t0 - W + 1;
  const int U = W + (pair ? 2 * WAVE : WAVE) - 1;   // <= N (the host picks EPL; rsr_pair)

  unsigned long long key[EPL];
  unsigned pos[EPL];
  bool num[EPL];
  int c = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int u = lane * EPL + e;
    const int i = ubase + u;
    const double v = (u < U && i >= first && i < len) ? vol[i] : qnan();   // +-inf is a value to Series.quantile
    key[e] = okey_nan_last(v);
    num[e] = v == v;
    pos[e] = (unsigned)u;
    c += num[e] ? 1 : 0;
  }
  // exclusive prefix of the non-NaN counts in union order
  int incl = c;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int y = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += y;
  }
  wave_lds_fence();   // the previous step's reads are done before this step's writes
  {
    int run = incl - c;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      L.cnt[lane * EPL + e] = (unsigned short)run;
      run += num[e] ? 1 : 0;
    }
    if (lane == WAVE - 1) L.cnt[N] = (unsigned short)run;
  }

  // bitonic sort of (key, pos), ascending
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int d = k >> 1; d > 0; d >>= 1) {
      if (d < EPL) {   // partner in this lane's registers
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          if (e & d) continue;
          const int i = lane * EPL + e;
          const bool up = (i & k) == 0;
          const unsigned long long a = key[e], b = key[e + d];
          const bool swap = (up & (b < a)) | (!up & (a < b));   // selects, not branches
          key[e] = swap ? b : a;
          key[e + d] = swap ? a : b;
          const unsigned pa = pos[e], pb = pos[e + d];
          pos[e] = swap ? pb : pa;
          pos[e + d] = swap ? pa : pb;
        }
      } else {
        const int ld = d / EPL;   // partner lane distance
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int i = lane * EPL + e;
          const unsigned lo32 = lane_xor((unsigned)key[e], ld);
          const unsigned hi32 = lane_xor((unsigned)(key[e] >> 32), ld);
          const unsigned long long pk = ((unsigned long long)hi32 << 32) | lo32;
          const bool lower = (i & d) == 0, up = (i & k) == 0;
          const bool keep_min = lower == up;   // the lower slot of an ascending pair keeps the minimum
          const bool take = (keep_min & (pk < key[e])) | (!keep_min & (key[e] < pk));
          key[e] = take ? pk : key[e];
          const unsigned pp = lane_xor(pos[e], ld);
          pos[e] = take ? pp : pos[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    L.key[lane * EPL + e] = key[e];
    L.idx[pos[e]] = (unsigned char)(lane * EPL + e);   // pos is a permutation of 0 .. N - 1
  }
  wave_lds_fence();
  // one-hot masks of this lane's union slots, their XOR prefix in slot order: P[e] = X(lane * EPL + e)
  unsigned P[EPL][NWORD];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int j = L.idx[lane * EPL + e];
#pragma unroll
    for (int w = 0; w < NWORD; ++w) {
      const unsigned oh = (j >> 5) == w ? (1u << (j & 31)) : 0u;
      P[e][w] = e == 0 ? oh : (P[e - 1][w] ^ oh);
    }
  }
#pragma unroll
  for (int w = 0; w < NWORD; ++w) {
    const unsigned tot = P[EPL - 1][w];
    const unsigned excl = wave_scan_xor(tot, lane) ^ tot;
#pragma unroll
    for (int e = 0; e < EPL; ++e) P[e][w] ^= excl;
  }

  // the floors of the step `off` candles after the sorted one: lane's window is union slots [off + lane, off + lane + W)
  auto pick = [&](int off) {
    wave_lds_fence();   // the reads of the pick before are done
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int jl = lane * EPL + e - off + 1, jh = lane * EPL + e - off - (W - 1);
#pragma unroll
      for (int w = 0; w < NWORD; ++w) {
        if (jl >= 0 && jl < WAVE) L.Xlo[jl][w] = P[e][w];
        if (jh >= 0 && jh < WAVE) L.Xhi[jh][w] = P[e][w];
      }
    }
    wave_lds_fence();
    double r = qnan();
    const int n = (int)L.cnt[off + lane + W] - (int)L.cnt[off + lane];
    if (n > 0) {
      unsigned M[NWORD];
#pragma unroll
      for (int w = 0; w < NWORD; ++w) M[w] = L.Xhi[lane][w] ^ (off + lane > 0 ? L.Xlo[lane][w] : 0u);
      // np.percentile(method="linear"): bq_select.hip's virtual index and two-sided lerp
      const double vi = (double)(n - 1) * q;
      const double fl = floor(vi);
      const int prev = (int)fl;
      const int nxt = prev + 1 < n ? prev + 1 : n - 1;
      const double gamma = vi - fl;
      const double a = okey_value(L.key[select_bit<NWORD>(M, prev)]);
      const double b = okey_value(L.key[select_bit<NWORD>(M, nxt)]);
      const double d = b - a;
      r = gamma >= 0.5 ? b - d * (1.0 - gamma) : a + d * gamma;
    }
    return r;
  };
  const double r = pick(0);
  if (pair) next = pick(WAVE);
  return r;
}

// Five waves a SIMD is what <4>'s LDS allows; left alone the allocator takes 101 VGPRs there (4 waves). <2> needs
// no such bound (57 VGPRs, 8 waves): the attribute's minimum does not change its code.
template <int EPL>
__global__ __launch_bounds__(RP_NT) __attribute__((amdgpu_waves_per_eu(5))) void rs_reversal_kernel(const RsrArgs A) {
  __shared__ RsrLds<EPL> lds_all[RP_WPB];
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  RsrLds<EPL>& L = lds_all[__builtin_amdgcn_readfirstlane(threadIdx.x / WAVE)];
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const double* __restrict__ vol = A.volume + s * A.ld_v;
  // omask bit k: a BQ_RSR_V_*
  ReplayOut<RsrArgs, BQ_RSR_NVALUES> O(A.status, A.ld_out, s, lane);
#pragma unroll
  for (int k = 0; k < BQ_RSR_NVALUES; ++k) O.set(k, A.val[k]);

  // one step's columns, candle tb + lane (NaN / absent past the panel's end)
  auto load_step = [&](int tb) {
    const int u = tb + lane;
    const bool in = u < T;
    const Karg<RsrArgs> K = kernarg<RsrArgs>();
    const unsigned ci = ctx_index(K, u, T);
    const int64_t si = sym_index(K, s, u, T);
    const uint8_t* cokp = K->ctx_ok;
    const uint8_t* fokp = K->feat_ok;
    const int8_t* mkp = K->regime;
    const double* arp = K->avg_ret;
    const double* rsp = K->rs;
    RsrStep x;
    x.v = in ? vol[u] : qnan();
    x.cok = cokp ? cokp[ci] != 0 : true;
    x.mk = mkp[ci];
    x.ar = arp[ci];
    x.fok = fokp ? fokp[si] != 0 : true;
    x.rs = rsp[si];
    return x;
  };

  const int b0 = R.b0();
  const bool any = R.any();
  double carry = qnan();   // this step's floors, where the step before sorted for both
  bool carried = false;    // wave-uniform
  RsrStep cur = {};
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    if (!any || t0 + WAVE <= from || t0 >= len) {   // no replayed candle in this step
      if (t < T) O.no_frame(t0, BQ_RSR_NO_FRAME);
      carried = false;
      continue;
    }
    if (t0 == b0) cur = load_step(t0);
    RsrStep nxt = cur;
    if (t0 + WAVE < len) nxt = load_step(t0 + WAVE);   // in flight during this step's arithmetic
    const Karg<RsrArgs> K = kernarg<RsrArgs>();
    const auto& P = K->p;
    const int W = P.window;

    // ---- the gates, in the method's order
    int st = BQ_RSR_EMIT;
    if (!(t >= from && t < len)) st = BQ_RSR_NO_FRAME;
    else if (t + 1 - first < W) st = BQ_RSR_SHORT_FRAME;                // :85
    else if (!cur.cok) st = BQ_RSR_NO_CONTEXT;                           // :61
    else if (cur.mk < 0) st = BQ_RSR_REGIME_NONE;                        // :63
    else if (cur.mk != BQ_RSR_REGIME_RANGE) st = BQ_RSR_NOT_RANGE;       // :65
    else if (cur.ar >= P.avg_return_max) st = BQ_RSR_MARKET_NOT_WEAK;    // :67, a NaN goes on
    else if (!cur.fok) st = BQ_RSR_NO_FEATURES;                          // :69
    else if (cur.rs <= P.rs_min) st = BQ_RSR_RS_INSUFFICIENT;            // :71, a NaN goes on
    const bool reach = st == BQ_RSR_EMIT;

    double floor_v = qnan();
    const bool have = carried;
    carried = false;
    if (__ballot(reach)) {   // wave-uniform: :97-98 for the step's candles
      double f = carry;
      if (!have) {
        carried = rsr_pair<EPL>(W) && t0 + WAVE < len;   // the next step has a candle of the frame: sort for both
        f = rsr_floor<EPL>(L, vol, t0, first, len, W, P.quantile, lane, carried, carry);
      }
      if (reach) floor_v = f;
      if (reach && cur.v <= floor_v) st = BQ_RSR_DEAD_TAPE;   // :100, a NaN on either side goes on
    }
    if (t < T) {
      O.st[t0] = (uint8_t)st;
      if (O.has(BQ_RSR_V_FLOOR)) O.val[BQ_RSR_V_FLOOR][t0] = floor_v;
    }
    cur = nxt;
  }
}

}  // namespace bq

extern "C" void bq_rs_reversal_default_params(bq_rs_reversal_params* p) {
  if (!p) return;
  // RelativeStrengthReversalRange's class attributes (:38-41)
  p->window = 96;
  p->reserved = 0;
  p->quantile = 0.20;
  p->avg_return_max = -0.02;
  p->rs_min = 0.05;
}

extern "C" int bq_rs_reversal_replay(const double* volume, int64_t ld_v, const uint8_t* context_ok,
                                     const int8_t* market_regime, const double* average_return, int64_t ctx_T,
                                     const uint8_t* features_ok, const double* relative_strength_vs_btc,
                                     int64_t ld_sym, const int64_t* lens, const int64_t* first_t,
                                     const int64_t* from_t, int64_t S, int64_t T,
                                     const bq_rs_reversal_params* params, uint8_t* status, double* const* values,
                                     int64_t ld_out, void* stream) {
  using namespace bq;
  if (!volume || !market_regime || !average_return || !relative_strength_vs_btc || !status || S < 0 || T < 0 ||
      ld_v < T || ld_out < T || (ld_sym != 0 && ld_sym < T) || (ctx_T != 1 && ctx_T != T) ||
      T > 0x7fffffff - 2 * WAVE)
    return BQ_EINVAL;
  RsrArgs A;
  memset(&A, 0, sizeof(A));
  if (params) A.p = *params;
  else bq_rs_reversal_default_params(&A.p);
  const bq_rs_reversal_params& p = A.p;
  if (!all_finite({p.avg_return_max, p.rs_min})) return BQ_EINVAL;
  if (p.window < 1 || p.window > BQ_RSR_MAX_WINDOW || !(p.quantile >= 0.0 && p.quantile <= 1.0)) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  // Series.quantile hands numpy the percentile q * 100, which numpy divides by 100: for some q another double
  A.p.quantile = p.quantile * 100.0 / 100.0;
  int64_t blocks;
  if (!replay_blocks(S, blocks)) return BQ_EINVAL;
  A.volume = volume;
  A.avg_ret = average_return;
  A.rs = relative_strength_vs_btc;
  A.ctx_ok = context_ok;
  A.feat_ok = features_ok;
  A.regime = market_regime;
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_v = ld_v;
  A.ld_sym = ld_sym;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.ctx_T = (int)ctx_T;
  A.status = status;
  replay_values(A.val, A.omask, values);
  const dim3 grid((unsigned)blocks), block(RP_NT);
  hipStream_t st = (hipStream_t)stream;
  // window + 63 union slots: 128 hold a window of up to 65
  if (p.window + WAVE - 1 <= 2 * WAVE) hipLaunchKernelGGL((rs_reversal_kernel<2>), grid, block, 0, st, A);
  else hipLaunchKernelGGL((rs_reversal_kernel<4>), grid, block, 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
