// FailedSpikeFade.latest_signal() of EVERY frame of a row (gfx950;
// strategies/failed_spike_fade.py:229-594): column t of row s = the method on
// a fresh instance whose frame is df.iloc[first_t[s]:t + 1]. Two steps of
// detect() are frame-wide — auto_calibrate's two np.quantile calls (:229-257)
// and apply_cooldown's greedy walk over labels formed under them (:495-520) —
// so a whole-row pass is right on a frame's newest column only. Two facts make
// every column cheap (checked against the real class,
// tests/golden/spikeframes.npz):
//   a. only the two calibrated scalars theta_t = (vcmr_t, pbbt_t) are
//      frame-wide. Given them, the labels of a row u <= t are element-wise in
//      columns that are the same in every frame holding u (the inputs here),
//      looking one row ahead (the 'last' label mode's shift(-1): NaN at u = t)
//      and up to 30 rows back (the cluster count, the 3-bar volume condition).
//   b. the cooldown walk may start at any run of `bars` rows without a
//      preliminary label: the first label after it is kept whatever came before.
//
// spike_prefix_quantile_kernel: the expanding np.quantile of volume_ratio and
//   price_change_abs at every t. One 2-wave workgroup per row, one wave per
//   column: the wave keeps the prefix's order keys SORTED in LDS and inserts
//   candle t's key by one top-down sweep (64 keys per step: those above the
//   new key move up one slot, the sweep stops at the first chunk that holds a
//   key <= it). The two order statistics of numpy's 'linear' method are then
//   two broadcast LDS reads, lerped by bq_row_quantile's own helper
//   (quantile_pos / quantile_lerp: the same bits). NaN is no observation, +-inf
//   is one. About n / 128 + 1 chunk moves per insert: T^2 / 256 for a row, 625
//   at the live store's T = 400, 16 384 at the cap of 2048 candles (8 B keys:
//   32 KiB of LDS per workgroup, 4-5 workgroups per CU). Lanes of one DS
//   instruction touch consecutive 8-byte slots: no bank conflicts. The raw
//   quantiles go to the workspace, with each column's first observed candle
//   (the calibration is skipped while either distribution is empty).
//
// spike_frames_kernel: the wave-per-row replay mapping (bq_replay.h). Lane i
//   holds candle t = t0 + i, forms theta_t from the two raw quantiles and the
//   flags of row t under theta_t (spike_eval: 10 neighbouring volume ratios by
//   default, L1 hits, and nine other loads). Columns whose preliminary label
//   is set (rare) are then served one at a time: the 64 lanes evaluate
//   label_pre(u; theta_t) for u = t - 63 .. t, one ballot; a scan of that mask
//   from t - 1 down finds the nearest run of `bars` clear rows, and the greedy
//   rule replays forward from it inside the same mask. While no run is found
//   and the frame's first row is not reached the block moves back by 64; the
//   forward replay then re-evaluates from the run. The long and the short
//   label are walked separately, as the method does.
//   Resource usage (gfx950 cross-compile, -O3): see DESIGN.md §4.29.
#include "bq_spikeframes.h"

namespace bq {

__global__ __launch_bounds__(SF_QNT) void spike_prefix_quantile_kernel(const SpikeFramesArgs A) {
  extern __shared__ uint64_t sf_keys[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int64_t s = blockIdx.x;
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  int* fo_out = A.first_obs + 2 * s + wv;
  if (!R.any()) {
    if (lane == 0) *fo_out = T;
    return;
  }
  uint64_t* sk = sf_keys + (int64_t)wv * A.cap;   // n <= len - first <= T <= cap sorted keys
  const double* __restrict__ x = A.in[wv ? BQ_SF_PRICE_CHANGE_ABS : BQ_SF_VOLUME_RATIO] + s * A.ld_in -
                                 (A.aligned ? first : 0);
  double* __restrict__ qo = (wv ? A.qp : A.qv) + s * (int64_t)T;
  const double q = wv ? A.p.price_base_floor_quantile : A.p.volume_quantile;
  int n = 0, fo = T;
  for (int t0 = R.e0(); t0 < len; t0 += WAVE) {
    const int t = t0 + lane;
    const bool in = t >= first && t < len;
    const double xv = in ? x[t] : qnan();
    double res = qnan();
    const int i0 = first > t0 ? first - t0 : 0, i1 = len - t0 < WAVE ? len - t0 : WAVE;
    for (int i = i0; i < i1; ++i) {
      const double xi = readlane_f64(xv, i);
      if (xi == xi) {   // wave-uniform
        const uint64_t key = order_key(xi);
        int pos = 0;
        for (int base = (n - 1) & ~(WAVE - 1); n > 0 && base >= 0; base -= WAVE) {
          const int p = base + lane;
          const bool have = p < n;
          const uint64_t k = have ? sk[p] : 0ull;
          const bool gt = have && k > key;
          if (gt) sk[p + 1] = k;   // p + 1 <= n <= T - 1 < cap
          const uint64_t le = __ballot(have && !gt);
          if (le) {
            pos = base + 64 - __builtin_clzll(le);
            break;
          }
        }
        if (lane == 0) sk[pos] = key;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (n == 0) fo = t0 + i;
        ++n;
      }
      if (t0 + i >= from && n > 0) {
        const QuantilePos qp = quantile_pos(n, q);
        const double a = key_value(sk[qp.prev]), b = key_value(sk[qp.next]);   // prev <= next <= n - 1
        const double r = quantile_lerp(a, b, qp.gamma);
        if (lane == i) res = r;
      }
    }
    if (in && t >= from) qo[t] = res;
  }
  if (lane == 0) *fo_out = fo;
}

__global__ __launch_bounds__(RP_NT) void spike_frames_kernel(const SpikeFramesArgs A) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = replay_row_index();
  if (s >= A.S) return;   // whole wave
  const auto k = kernarg<SpikeFramesArgs>();
  const int T = A.T;
  const ReplayRow R = replay_row(A.lens, A.first, A.from, s, T);
  const int len = R.len, first = R.first, from = R.from;
  const int64_t off = s * A.ld_in - (A.aligned ? first : 0), offb = s * A.ld_b - (A.aligned ? first : 0);
  SpikeFramesRow P;
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
  const uint8_t* __restrict__ upw = A.in_b[BQ_SF_IN_UPWARD] + offb;
  const uint8_t* __restrict__ dnw = A.in_b[BQ_SF_IN_DOWNWARD] + offb;
  const double* __restrict__ qv = A.qv + s * (int64_t)T;
  const double* __restrict__ qp = A.qp + s * (int64_t)T;
  const int fo0 = A.first_obs[2 * s], fo1 = A.first_obs[2 * s + 1];
  const int obs_from = fo0 > fo1 ? fo0 : fo1;   // both distributions hold an observation from here on
  const int bars = A.p.post_spike_cooldown_bars;
  const int64_t orow = s * A.ld_out;
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    const bool valid = R.any() && t >= from && t < len;
    double vc = qnan(), pb = qnan();
    unsigned bits = 0u;
    bool acc = false, accs = false, up = false, down = false;
    if (__ballot(valid)) {
      if (valid) {
        // auto_calibrate on a fresh instance (:236-247); skipped while a distribution is empty
        vc = k->p.volume_cluster_min_ratio;
        pb = k->p.price_break_base_threshold;
        if (t >= obs_from) {
          const double a = qv[t], b = qp[t];
          const double mv = k->p.min_volume_ratio, mf = k->p.min_price_abs_floor;
          vc = a > mv ? a : mv;                 // max(min_volume_ratio, quantile)
          const double fl = b > mf ? b : mf;    // max(min_price_abs_floor, quantile)
          pb = fl > pb ? fl : pb;               // max(old_price_floor, new_price_floor)
        }
        bits = spike_eval(P, k, t, t, vc, pb);
        acc = P.acc[t] != 0;
        accs = P.accs[t] != 0;
        up = upw[t] != 0;
        down = dnw[t] != 0;
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
          if (spike_cooldown_keeps(P, k, t0 + i, readlane_f64(vc, i), readlane_f64(pb, i), bit, bars, lane))
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
          (bits & SF_PBF) != 0u, (bits & SF_CUM) != 0u, (bits & SF_CUMS) != 0u, acc, accs, up, down};
#pragma unroll
      for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_OUT; ++j)
        if ((om >> j) & 1) k->out_b[j][orow + t] = (uint8_t)vals[j];
      if ((om >> BQ_NUM_SPIKE_FRAMES_OUT) & 1) k->vcmr[orow + t] = vc;
      if ((om >> (BQ_NUM_SPIKE_FRAMES_OUT + 1)) & 1) k->pbbt[orow + t] = pb;
    }
  }
}

}  // namespace bq

extern "C" void bq_spike_frames_default_params(bq_spike_frames_params* p) {
  if (!p) return;
  // FailedSpikeFade's attributes (:66-91) and auto_calibrate's defaults (:229-235)
  p->volume_cluster_window = 8;
  p->volume_cluster_min_count = 2;
  p->cumulative_price_window = 3;
  p->label_mode = 0;
  p->require_both_patterns = 0;
  p->require_bullish_spike = 1;
  p->post_spike_cooldown_bars = 8;
  p->reserved = 0;
  p->cumulative_price_threshold = 0.025;
  p->body_size_pct_min = 0.005;
  p->volume_cluster_min_ratio = 1.6;
  p->price_break_base_threshold = 0.03;
  p->volume_quantile = 0.97;
  p->price_base_floor_quantile = 0.75;
  p->min_volume_ratio = 1.15;
  p->min_price_abs_floor = 0.015;
}

extern "C" size_t bq_spike_frames_workspace(int64_t S, int64_t T) {
  if (S <= 0 || T <= 0) return 0;
  return (size_t)S * (size_t)T * 2 * sizeof(double) + (size_t)S * 2 * sizeof(int);
}

extern "C" int bq_spike_frames(const double* const* in, int64_t ld_in, const uint8_t* const* in_b, int64_t ld_b,
                               int32_t aligned, const int64_t* lens, const int64_t* first_t, const int64_t* from_t,
                               int64_t S, int64_t T, const bq_spike_frames_params* params, void* workspace,
                               size_t workspace_bytes, double* vcmr, double* pbbt, uint8_t* const* out_b,
                               int64_t ld_out, void* stream) {
  using namespace bq;
  SpikeFramesArgs A;
  const int st0 = spike_frames_setup(A, in, ld_in, in_b, ld_b, aligned, lens, first_t, from_t, S, T,
                                     BQ_SPIKE_FRAMES_MAX_T, params, vcmr, pbbt, out_b, ld_out);
  if (st0 != BQ_OK) return st0;
  if (S == 0 || T == 0) return BQ_OK;
  if (!workspace || workspace_bytes < bq_spike_frames_workspace(S, T) || ((uintptr_t)workspace & 7)) return BQ_EINVAL;
  int64_t blocks;
  if (!replay_blocks(S, blocks) || S > 0x7fffffff) return BQ_EINVAL;
  A.cap = (int)((T + WAVE - 1) / WAVE) * WAVE;
  A.qv = (double*)workspace;
  A.qp = A.qv + S * T;
  A.first_obs = (int*)(A.qp + S * T);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)2 * A.cap * sizeof(uint64_t);   // <= 32 KiB
  hipLaunchKernelGGL(spike_prefix_quantile_kernel, dim3((unsigned)S), dim3(SF_QNT), lds, st, A);
  if (hipGetLastError() != hipSuccess) return BQ_EHIP;
  hipLaunchKernelGGL(spike_frames_kernel, dim3((unsigned)blocks), dim3(RP_NT), 0, st, A);
  return hipGetLastError() == hipSuccess ? BQ_OK : BQ_EHIP;
}
