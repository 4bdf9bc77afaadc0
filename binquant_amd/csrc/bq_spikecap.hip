// FailedSpikeFade.latest_signal() of every frame of a row under a SLIDING frame
// cap (gfx950; bq_spike_frames_capped): column t of row s = the
// method on a fresh instance whose frame is df.iloc[max(first, t + 1 -
// frame_cap):t + 1], the frame the live store hands a strategy. bq_spikeframes.hip's
// fact a. (given the two calibrated scalars, a row's labels are element-wise in
// columns that every frame holding the row shares) then holds only deep in a
// frame: near its first row the columns are the frame's own (the header's rule
// table).
//
// spike_sliding_quantile_kernel keeps the FRAME's keys sorted in LDS (at most
//   frame_cap a column, whatever T): an insert per candle and the erase of what
//   leaves the frame.
// spike_frames_capped_kernel is spike_frames_kernel with spike_eval<true> /
//   spike_cooldown_keeps<true> (bq_spikeframes.h), which restate the frame-local
//   columns from the row's and stop the walk at the frame's first row. The
//   uncapped kernels are the <false> instantiations; they live in their own
//   file so that their device code stays what it was (make isa-digest).
#include "bq_spikeframes.h"

namespace bq {

struct SpikeCapArgs : SpikeFramesArgs {
  const int32_t* in_i[BQ_NUM_SPIKE_FRAMES_IN_I];
  int64_t ld_i;
  bq_spike_frames_cap c;
  uint8_t* cal;   // workspace: [2][S][T] the column's set holds an observation at t
};

// A wave's sorted keys sk[0 .. n): insert by the top-down sweep of spike_prefix_quantile_kernel (sk[n] is a slot).
__device__ __forceinline__ void sorted_insert(uint64_t* sk, int& n, uint64_t key, int lane) {
  int pos = 0;
  for (int base = (n - 1) & ~(WAVE - 1); n > 0 && base >= 0; base -= WAVE) {
    const int p = base + lane;
    const bool have = p < n;
    const uint64_t k = have ? sk[p] : 0ull;
    const bool gt = have && k > key;
    if (gt) sk[p + 1] = k;
    const uint64_t le = __ballot(have && !gt);
    if (le) {
      pos = base + 64 - __builtin_clzll(le);
      break;
    }
  }
  if (lane == 0) sk[pos] = key;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  ++n;
}

// Erase one key equal to `key` (present; equal keys are interchangeable): every key above it moves down one
// slot, top-down like the insert, which overwrites the highest slot that holds a key <= `key`. A chunk's lowest
// lane writes the last slot of the chunk below, so that chunk is read first.
__device__ __forceinline__ void sorted_erase(uint64_t* sk, int& n, uint64_t key, int lane) {
  if (n <= 0) return;
  int base = (n - 1) & ~(WAVE - 1);
  uint64_t k = base + lane < n ? sk[base + lane] : 0ull;
  for (;;) {
    const int p = base + lane;
    const bool have = p < n;
    const bool gt = have && k > key;
    const uint64_t below = base > 0 ? sk[p - WAVE] : 0ull;   // 0 <= p - WAVE < n
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (gt && p > 0) sk[p - 1] = k;
    if (__ballot(have && !gt) || base == 0) break;
    base -= WAVE;
    k = below;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  --n;
}

// The np.quantile of volume_ratio (wave 0) and price_change_abs (wave 1) over every capped frame of a row: the
// frame's keys sorted in LDS (at most frame_cap - 1 before a candle's insert), one insert per candle and, once
// the frame slides, the erase of what leaves it — volume_ratio at row f + base_window - 1 of the frame left
// behind; price_change_abs on rows f + 1 .. g' when the row leaving, f, held the frame's first valid close (g'
// the next one: a run of rows when closes are missing). A row is walked from max(first, from + 1 - frame_cap):
// the frames before `from` are not formed, so the window is rebuilt by at most frame_cap - 1 inserts.
__global__ __launch_bounds__(SF_QNT) void spike_sliding_quantile_kernel(const SpikeCapArgs A) {
  extern __shared__ uint64_t sfc_keys[];
  constexpr int NONE = 0x7fffffff;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int64_t s = blockIdx.x;
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  if (!R.any()) return;   // spike_frames_capped_kernel reads nothing of such a row
  const int len = R.len, first = R.first, from = R.from;
  const int M = A.c.frame_cap, bw = A.c.base_window;
  const int ts = from + 1 - M > first ? from + 1 - M : first;
  uint64_t* sk = sfc_keys + (int64_t)wv * A.cap;
  const int64_t off = s * A.ld_in - (A.aligned ? first : 0);
  const double* __restrict__ x = A.in[wv ? BQ_SF_PRICE_CHANGE_ABS : BQ_SF_VOLUME_RATIO] + off;
  const double* __restrict__ cl = A.in[BQ_SF_CLOSE] + off;
  double* __restrict__ qo = (wv ? A.qp : A.qv) + s * (int64_t)T;
  uint8_t* __restrict__ cal = A.cal + ((int64_t)wv * A.S + s) * T;
  const double q = wv ? A.p.price_base_floor_quantile : A.p.volume_quantile;
  const int lag = wv ? M - 1 : M - bw + 1;   // step t's leaving row: t - lag (1 <= lag <= M)
  int n = 0, g = NONE;                       // g: the frame's first valid close (wave 1)
  for (int t0 = ts & ~(WAVE - 1); t0 < len; t0 += WAVE) {
    const int t = t0 + lane;
    const bool in = t >= ts && t < len;
    const bool slid = in && t - M >= ts;   // the frame's first row moves from t - M to t + 1 - M at this step
    const double xv = in ? x[t] : qnan();
    const double xl = slid ? x[t - lag] : qnan();                // ts < t - lag <= t
    const double cn = slid && wv ? cl[t - M + 1] : qnan();
    const double cv = in && wv ? cl[t] : qnan();
    double res = qnan();
    bool has = false;
    const int i0 = ts > t0 ? ts - t0 : 0, i1 = len - t0 < WAVE ? len - t0 : WAVE;
    for (int i = i0; i < i1; ++i) {
      const int tt = t0 + i;
      if (tt - M >= ts) {   // wave-uniform, like everything below
        if (!wv) {
          const double xi = readlane_f64(xl, i);
          if (xi == xi) sorted_erase(sk, n, order_key(xi), lane);
        } else if (g == tt - M) {
          double pw = readlane_f64(xl, i), cw = readlane_f64(cn, i);
          for (int w = tt - M + 1;;) {
            if (w >= tt) {   // no valid close before this candle
              g = NONE;
              break;
            }
            if (pw == pw) sorted_erase(sk, n, order_key(pw), lane);
            if (cw == cw) {
              g = w;
              break;
            }
            ++w;   // <= tt < len
            pw = x[w];
            cw = cl[w];
          }
        }
      }
      const double xi = readlane_f64(xv, i);
      bool ins = xi == xi;
      if (!wv) {
        const int f = tt + 1 - M > ts ? tt + 1 - M : ts;
        ins = ins && tt >= f + bw - 1;
      } else if (g == NONE) {
        const double ci = readlane_f64(cv, i);
        if (ci == ci) g = tt;
        ins = false;
      } else {
        ins = ins && g < tt;
      }
      if (ins && n < A.cap) sorted_insert(sk, n, order_key(xi), lane);   // n <= frame_cap - 1 < A.cap before it
      if (tt >= from) {
        if (n > 0) {
          const QuantilePos qp = quantile_pos(n, q);
          const double a = key_value(sk[qp.prev]), b = key_value(sk[qp.next]);   // prev <= next <= n - 1
          const double r = quantile_lerp(a, b, qp.gamma);
          if (lane == i) res = r;
        }
        if (lane == i) has = n > 0;
      }
    }
    if (in && t >= from) {
      qo[t] = res;
      cal[t] = has ? 1 : 0;
    }
  }
}

// spike_frames_kernel on the capped frames: lane i forms candle t's frame [f, t], g and theta_t, then the same
// flags and walk with the frame-local rules of spike_eval<true>.
__global__ __launch_bounds__(RP_NT) void spike_frames_capped_kernel(const SpikeCapArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const auto k = kernarg<SpikeCapArgs>();
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const int shift = A.aligned ? first : 0;
  const int64_t off = s * A.ld_in - shift, offb = s * A.ld_b - shift, offi = s * A.ld_i - shift;
  SpikeCapRow P;
  P.vr = A.in[BQ_SF_VOLUME_RATIO] + off;
  P.pca = A.in[BQ_SF_PRICE_CHANGE_ABS] + off;
  P.dyn = A.in[BQ_SF_DYN_THRESHOLD] + off;
  P.bsp = A.in[BQ_SF_BODY_SIZE_PCT] + off;
  P.cp = A.in[BQ_SF_CUM_POS] + off;
  P.cn = A.in[BQ_SF_CUM_NEG] + off;
  P.op = A.in[BQ_SF_OPEN] + off;
  P.cl = A.in[BQ_SF_CLOSE] + off;
  P.acc = A.in_b[BQ_SF_IN_ACCEL] + offb;
  P.accs = A.in_b[BQ_SF_IN_ACCEL_SHORT] + offb;
  P.first = first;
  P.dsrc = A.in_i[BQ_SF_DYN_SRC] + offi;
  P.cnext = A.in_i[BQ_SF_CLOSE_NEXT] + offi;
  P.shift = shift;
  // the zone's two columns and the candle-indexed flags in VGPRs: the walk's masks and the row's other
  // pointers fill the SGPR file (bq_replay.h's ReplayOut does the same)
  asm volatile("" : "+v"(P.dsrc), "+v"(P.cnext), "+v"(P.acc), "+v"(P.accs), "+v"(P.bsp), "+v"(P.cp), "+v"(P.cn), "+v"(P.op),
               "+v"(P.cl), "+v"(P.dyn));
  const int bars = A.p.post_spike_cooldown_bars;
  const int64_t orow = s * A.ld_out;
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    const bool valid = R.any() && t >= from && t < len;
    double vc = qnan(), pb = qnan();
    unsigned bits = 0u;
    bool up = false, down = false;
    SpikeFrame F{0, 0};
    if (__ballot(valid)) {
      if (valid) {
        // what only this row of the step reads: pointers through kernarg(), not held across the walk
        const int64_t wt = s * (int64_t)T + t;
        const double* qv = k->qv + wt;
        const double* qp = k->qp + wt;
        const uint8_t* calv = k->cal + wt;
        const uint8_t* calp = calv + k->S * (int64_t)T;
        const uint8_t* upw = k->in_b[BQ_SF_IN_UPWARD] + offb + t;
        const uint8_t* dnw = k->in_b[BQ_SF_IN_DOWNWARD] + offb + t;
        const int M = k->c.frame_cap;
        F.f = t + 1 - M > first ? t + 1 - M : first;
        const int g = P.cnext[F.f] + shift;
        F.g = g > F.f ? g : F.f;   // close_next[j] >= j
        // auto_calibrate on a fresh instance (:236-247); skipped while a distribution is empty in the frame
        vc = k->p.volume_cluster_min_ratio;
        pb = k->p.price_break_base_threshold;
        if (*calv != 0 && *calp != 0) {
          const double a = *qv, b = *qp;
          const double mv = k->p.min_volume_ratio, mf = k->p.min_price_abs_floor;
          vc = a > mv ? a : mv;
          const double fl = b > mf ? b : mf;
          pb = fl > pb ? fl : pb;
        }
        bits = spike_eval<true>(P, k, t, t, vc, pb, F);
        up = *upw != 0;     // the streaks' rolling(n) window lies inside a full frame (n <= 64)
        down = *dnw != 0;
      }
    }
    bool label = (bits & SF_PRE) != 0u, label_s = (bits & SF_SPRE) != 0u;
    if (bars > 0) {
      for (int side = 0; side < 2; ++side) {
        const unsigned bit = side ? SF_SPRE : SF_PRE;
        uint64_t need = __ballot((bits & bit) != 0u);
        uint64_t kept = 0ull;
        while (need) {   // wave-uniform: one column at a time
          const int i = __builtin_ctzll(need);
          need &= need - 1;
          const SpikeFrame Fi{__builtin_amdgcn_readlane(F.f, i), __builtin_amdgcn_readlane(F.g, i)};
          if (spike_cooldown_keeps<true>(P, k, t0 + i, readlane_f64(vc, i), readlane_f64(pb, i), bit, bars, lane, Fi))
            kept |= 1ull << i;
        }
        const bool kb = (kept >> lane) & 1ull;
        if (side) label_s = kb;
        else label = kb;
      }
    }
    if (t < T) {
      const int om = k->omask;
      const bool vals[BQ_NUM_SPIKE_FRAMES_OUT] = {
          label, (bits & SF_PRE) != 0u, label_s, (bits & SF_SPRE) != 0u, (bits & SF_VCF) != 0u,
          (bits & SF_PBF) != 0u, (bits & SF_CUM) != 0u, (bits & SF_CUMS) != 0u, (bits & SF_ACC) != 0u,
          (bits & SF_ACCS) != 0u, up, down};
#pragma unroll
      for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_OUT; ++j)
        if ((om >> j) & 1) k->out_b[j][orow + t] = (uint8_t)vals[j];
      if ((om >> BQ_NUM_SPIKE_FRAMES_OUT) & 1) k->vcmr[orow + t] = vc;
      if ((om >> (BQ_NUM_SPIKE_FRAMES_OUT + 1)) & 1) k->pbbt[orow + t] = pb;
    }
  }
}

}  // namespace bq

extern "C" size_t bq_spike_frames_capped_workspace(int64_t S, int64_t T) {
  if (S <= 0 || T <= 0) return 0;
  const size_t cells = (size_t)S * (size_t)T;
  return cells * 2 * sizeof(double) + ((cells * 2 + 7) & ~(size_t)7);
}

extern "C" int bq_spike_frames_capped(const double* const* in, int64_t ld_in, const uint8_t* const* in_b,
                                      int64_t ld_b, const int32_t* const* in_i, int64_t ld_i, int32_t aligned,
                                      const int64_t* lens, const int64_t* first_t, const int64_t* from_t, int64_t S,
                                      int64_t T, const bq_spike_frames_params* params,
                                      const bq_spike_frames_cap* cap, void* workspace, size_t workspace_bytes,
                                      double* vcmr, double* pbbt, uint8_t* const* out_b, int64_t ld_out,
                                      void* stream) {
  using namespace bq;
  SpikeCapArgs A;
  const int st0 = spike_frames_setup(A, in, ld_in, in_b, ld_b, aligned, lens, first_t, from_t, S, T,
                                     (int64_t)1 << 30, params, vcmr, pbbt, out_b, ld_out);
  if (st0 != BQ_OK) return st0;
  if (!cap || cap->frame_cap < BQ_SPIKE_FRAMES_MIN_CAP || cap->frame_cap > BQ_SPIKE_FRAMES_MAX_T ||
      cap->base_window < 1 || cap->base_window > BQ_SPIKE_FRAMES_MAX_WINDOW || cap->accel_volume_deriv_window < 1 ||
      cap->accel_volume_deriv_window > BQ_SPIKE_FRAMES_MAX_WINDOW ||
      !(cap->price_break_dynamic_q >= 0.0 && cap->price_break_dynamic_q <= 1.0) || !in_i || ld_i < T)
    return BQ_EINVAL;
  for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_IN_I; ++j)
    if (!(A.in_i[j] = in_i[j])) return BQ_EINVAL;
  if (S == 0 || T == 0) return BQ_OK;
  if (!workspace || workspace_bytes < bq_spike_frames_capped_workspace(S, T) || ((uintptr_t)workspace & 7))
    return BQ_EINVAL;
  int64_t blocks;
  if (!replay_blocks(S, blocks) || S > 0x7fffffff) return BQ_EINVAL;
  A.c = *cap;
  A.ld_i = ld_i;
  A.cap = (cap->frame_cap + WAVE - 1) / WAVE * WAVE;   // LDS slots per column: a frame's keys, whatever T
  A.qv = (double*)workspace;
  A.qp = A.qv + S * T;
  A.first_obs = nullptr;
  A.cal = (uint8_t*)(A.qp + S * T);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)2 * A.cap * sizeof(uint64_t);   // <= 32 KiB
  hipLaunchKernelGGL(spike_sliding_quantile_kernel, dim3((unsigned)S), dim3(SF_QNT), lds, st, A);
  if (hipGetLastError() != hipSuccess) return BQ_EHIP;
  hipLaunchKernelGGL(spike_frames_capped_kernel, dim3((unsigned)blocks), dim3(RP_NT), 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
