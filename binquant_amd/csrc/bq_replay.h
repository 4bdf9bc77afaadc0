// The wave-per-row mapping shared by the strategy replay kernels (bq_retest,
// bq_spikefade, bq_pricetracker, bq_meanrev, bq_rangefade): one wave walks a
// row in steps of 64 candles, lane i holding candle t0 + i, every column one
// coalesced load per step, the next step's columns loaded before this step's
// arithmetic. Candles max(from_t, first_t) .. lens - 1 of a row are replayed;
// a step that holds none of them is filled with the entry's NO_FRAME code.
// What a row carries from step to step (a state machine's entry, a ballot, a
// scan's carry) is wave-uniform. The step loop itself — the skip / fill
// branch, the warm-up call, the nxt / cur double buffer and the gates — stays
// written out in each kernel. Every helper is __forceinline__: a kernel built
// on them keeps the registers and occupancy of the hand-written copies they
// replaced and writes their bits. Internal to the library.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "bq_device.h"

namespace bq {

// ---- geometry ----------------------------------------------------------------
constexpr int RP_NT = 256;            // threads: RP_NT / WAVE rows per workgroup
constexpr int RP_WPB = RP_NT / WAVE;

// the wave's row; a wave with replay_row_index() >= S returns as a whole
__device__ __forceinline__ int64_t replay_row_index() {
  return (int64_t)blockIdx.x * RP_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
}

// b0 / e0 / any are formed where a kernel first uses them, not stored
struct ReplayRow {
  int64_t s;
  int len, first, from;   // clamped to [0, T]
  // the first step that holds a replayed candle / a candle of the frame; the row has a replayed candle
  __device__ __forceinline__ int b0() const { return from & ~(WAVE - 1); }
  __device__ __forceinline__ int e0() const { return first & ~(WAVE - 1); }
  __device__ __forceinline__ bool any() const { return from < len; }
};

// CLAMP_FROM: a candle before first_t has an empty frame and no message, so
// the replay starts at max(from_t, first_t). The retest replay marks those
// candles itself (SHORT_HISTORY) and takes from_t as given.
template <bool CLAMP_FROM = true>
__device__ __forceinline__ ReplayRow replay_row(const int64_t* lens, const int64_t* first, const int64_t* from,
                                                int64_t s, int T) {
  ReplayRow R;
  R.s = s;
  R.len = clamp_row(lens, s, T, T);
  R.first = clamp_row(first, s, 0, T);
  const int from0 = clamp_row(from, s, 0, T);
  R.from = (!CLAMP_FROM || from0 > R.first) ? from0 : R.first;
  return R;
}

// ---- the kernel's arguments, read where a step uses them -----------------------
// Thresholds, weights and ewm constants (up to ~75 dwords) are read from the
// kernarg segment through a pointer the compiler cannot see through: as loop
// invariants they would all be held in SGPRs beside the row pointers, and
// spill. They stay in the scalar cache.
template <class Args>
using Karg = const __attribute__((address_space(4))) Args*;

template <class Args>
__device__ __forceinline__ Karg<Args> kernarg() {
  Karg<Args> k = (Karg<Args>)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// ---- outputs -----------------------------------------------------------------
// The status column and the NV value columns as per-lane pointers held in
// VGPRs (candle `lane` of the row; a step adds t0), their presence as the bits
// of Args::omask: that many more row pointers and null flags would not fit
// the SGPR file beside the inputs'. Args has omask. The kernel hands the value
// columns over one by one, set(k, A.val[k]) under #pragma unroll: given a
// reference to the argument struct or to its val[] the compiler loads every
// kernel argument at entry (mean_reversion_kernel<true>: 4 SGPRs spilled).
template <class Args, int NV>
struct ReplayOut {
  uint8_t* st;
  double* val[NV];
  int64_t orow;   // the row's offset at candle `lane`

  __device__ __forceinline__ ReplayOut(uint8_t* status, int64_t ld_out, int64_t s, int lane) {
    orow = s * ld_out + lane;
    st = status + orow;
    asm volatile("" : "+v"(st));
  }
  __device__ __forceinline__ void set(int k, double* p) {
    val[k] = p + orow;
    asm volatile("" : "+v"(val[k]));
  }
  // bit k of omask: value column k is wanted (bits from NV on are the kernel's own)
  __device__ __forceinline__ bool has(int k) const { return (kernarg<Args>()->omask >> k) & 1; }
  // no replayed candle in this step (the caller tests t < T)
  __device__ __forceinline__ void no_frame(int t0, uint8_t code) const {
    st[t0] = code;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (has(k)) val[k][t0] = qnan();
  }
};

// ---- context rows and the symbol snapshot ---------------------------------------
// The index of candle t's context column (ctx_T 1: one column for all), as a
// VGPR: vector loads also where the context is one column.
template <class K>
__device__ __forceinline__ unsigned ctx_index(K k, int t, int T) {
  unsigned ci = k->ctx_T == 1 ? 0u : (unsigned)(t < T ? t : 0);
  asm volatile("" : "+v"(ci));
  return ci;
}

// rows 0 .. N - 1 of the context at column ci into x; returns ctx_ok there (NULL: present)
template <int N, class K>
__device__ __forceinline__ bool ctx_load(K k, unsigned ci, double (&x)[N]) {
  const unsigned ldc = (unsigned)k->ld_ctx;
  const uint8_t* cokp = k->ctx_ok;
  const double* ctxp = k->ctx;
  const bool cok = cokp ? cokp[ci] != 0 : true;
#pragma unroll
  for (int j = 0; j < N; ++j) x[j] = ctxp[j * ldc + ci];
  return cok;
}

// the index of row s's symbol-snapshot entry at candle t (ld_sym 0: one entry per row), as a VGPR
template <class K>
__device__ __forceinline__ int64_t sym_index(K k, int64_t s, int t, int T) {
  const int64_t lds = k->ld_sym;
  int64_t si = lds ? s * lds + (t < T ? t : 0) : s;
  asm volatile("" : "+v"(si));
  return si;
}

// ---- pandas' ewm(adjust=False).mean() formed in the pass -------------------------
// one constant set: pandas' alpha / old-weight factor om = 1 - alpha, the
// affine map y -> la y + lb x, apow[j] = la^(2^j)
struct Ewm {
  double alpha, om, la, lb;
  double apow[7];
};

inline void ewm_consts(Ewm& E, double alpha) {
  E.alpha = alpha;
  E.om = 1.0 - alpha;
  const double den = E.om + E.alpha;
  E.la = E.om / den;
  E.lb = E.alpha / den;
  E.apow[0] = E.la;
  for (int j = 1; j < 7; ++j) E.apow[j] = E.apow[j - 1] * E.apow[j - 1];
}
// pandas keeps com and forms alpha = 1 / (1 + com) from it: com = (span - 1) / 2 for ewm(span=),
// com = (1 - a) / a for ewm(alpha=a) with Wilder's a = 1 / window
inline double ewm_alpha_span(double span) { return 1.0 / (1.0 + (span - 1.0) / 2.0); }
inline double ewm_alpha_wilder(double window) {
  const double wa = 1.0 / window;
  return 1.0 / (1.0 + (1.0 - wa) / wa);
}

// NE series over NK constant sets. A Spec names, per series e: set(e) its
// constant set, seed(e) its seed candle first_t + seed(e) (1: a series of
// differences, NaN on the frame's first row), min_periods(e) whether the
// result is NaN until W observations; SWITCH: the series whose missing value
// turns the row serial.
template <int NE, int NK>
struct EwmState {
  double lpow[NK], rpow[NK];   // per lane: la^(lane + 1), la^((lane & 15) + 1)
  double carry[NE];            // the previous step's lane 63 (wave-uniform, in VGPRs)
  double swv[NE], sowt[NE];    // the serial recursion's weighted value and old weight
  int snobs[NE];               // and observation count (min_periods)
  bool serial;
};

// ew: the kernel argument's constant sets (read directly: once per row)
template <class Spec>
__device__ __forceinline__ void ewm_init(EwmState<Spec::NE, Spec::NK>& S, const Ewm* ew, int lane, bool on) {
#pragma unroll
  for (int k = 0; k < Spec::NK; ++k) S.lpow[k] = S.rpow[k] = 0.0;
#pragma unroll
  for (int e = 0; e < Spec::NE; ++e) {
    S.carry[e] = 0.0;
    S.swv[e] = qnan();
    S.sowt[e] = 1.0;
    S.snobs[e] = 0;
  }
  S.serial = false;
  if (on) {
#pragma unroll
    for (int k = 0; k < Spec::NK; ++k) {
      S.lpow[k] = pow_bits<7>(ew[k].apow, lane + 1);
      S.rpow[k] = pow_bits<5>(ew[k].apow, (lane & 15) + 1);
    }
  }
}

// Candles t0 .. t0 + 63 of the NE series into y (every lane executes it; called
// once for every step from first_t's on, in order). x[e]: the series' input at
// candle t0 + lane, +-inf already missing (win_val). ew: the constant sets
// through kernarg(). Each series is the affine map y -> la y + lb x: one DPP
// wave scan per step with the previous step's carry. A row that meets a
// missing x[SWITCH] inside its frame continues from that step with pandas' own
// recursion, serially over the step's lanes.
template <class Spec, class KEwm>
__device__ __forceinline__ void ewm_step(EwmState<Spec::NE, Spec::NK>& S, KEwm ew, const double (&x)[Spec::NE], int t0,
                                         int lane, int first, int len, int W, double (&y)[Spec::NE]) {
  constexpr int NE = Spec::NE, NK = Spec::NK;
  const int t = t0 + lane;
  const double xs = x[Spec::SWITCH];
  if (!S.serial && __ballot(t >= first && t < len && !(xs == xs))) {   // wave-uniform: the row turns serial here
    S.serial = true;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      // candles first + seed(e) .. t0 - 1 were all observations
      const int seed = first + Spec::seed(e);
      S.swv[e] = t0 > seed ? S.carry[e] : qnan();
      S.sowt[e] = 1.0;
      S.snobs[e] = t0 > seed ? t0 - seed : 0;
    }
  }
  if (S.serial) {   // pandas' recursion over the step, every series
    double om[NK], alpha[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      om[k] = ew[k].om;
      alpha[k] = ew[k].alpha;
    }
    const int i0 = first > t0 ? first - t0 : 0, n = len - t0 < WAVE ? len - t0 : WAVE;
#pragma unroll
    for (int e = 0; e < NE; ++e) y[e] = qnan();
    for (int i = i0; i < n; ++i) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int k = Spec::set(e);
        const double cur = readlane_f64(x[e], i);
        const bool obs = cur == cur;
        double wv = S.swv[e], owt = S.sowt[e];
        if (t0 + i == first) {
          wv = cur;
          owt = 1.0;
          if (Spec::min_periods(e)) S.snobs[e] = obs ? 1 : 0;
        } else {
          if (Spec::min_periods(e)) S.snobs[e] += obs ? 1 : 0;
          if (wv == wv) {
            owt *= om[k];
            if (obs) {
              if (wv != cur) {
                wv = owt * wv + alpha[k] * cur;
                wv /= owt + alpha[k];
              }
              owt = 1.0;
            }
          } else if (obs) {
            wv = cur;
          }
        }
        S.swv[e] = wv;
        S.sowt[e] = owt;
        asm volatile("" : "+v"(S.swv[e]), "+v"(S.sowt[e]));
        if (lane == i) y[e] = (Spec::min_periods(e) && S.snobs[e] < W) ? qnan() : wv;
      }
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int k = Spec::set(e);
    const int seed = first + Spec::seed(e);
    const double ap[5] = {ew[k].apow[0], ew[k].apow[1], ew[k].apow[2], ew[k].apow[3], ew[k].apow[4]};
    // zero before the seed, the seed itself: its lane receives a zero carry
    const double b = t < seed ? 0.0 : (t == seed ? x[e] : ew[k].lb * x[e]);
    const double inc = wave_scan_affine_dpp_rp(b, ap, S.rpow[k], lane);
    y[e] = fma(S.lpow[k], S.carry[e], inc);
    S.carry[e] = readlane_f64(y[e], WAVE - 1);
    asm volatile("" : "+v"(S.carry[e]));   // the series' uniform state lives in VGPRs, not beside the row pointers
    if (Spec::min_periods(e) && t - seed + 1 < W) y[e] = qnan();   // min_periods: t - seed + 1 observations so far
  }
}

// ---- host side of a launch -----------------------------------------------------
inline bool all_finite(std::initializer_list<double> v) {
  for (double x : v)
    if (!(x - x == 0.0)) return false;
  return true;
}

// workgroups for S rows; false where the grid would overflow
inline bool replay_blocks(int64_t S, int64_t& blocks) {
  blocks = (S + RP_WPB - 1) / RP_WPB;
  return blocks <= 0x7fffffff;
}

// val[k] = values[k] (values NULL: none) and their presence as the bits of omask
template <int NV>
inline void replay_values(double* (&val)[NV], int& omask, double* const* values) {
  for (int k = 0; k < NV; ++k) {
    val[k] = values ? values[k] : nullptr;
    omask |= val[k] ? 1 << k : 0;
  }
}

}  // namespace bq
