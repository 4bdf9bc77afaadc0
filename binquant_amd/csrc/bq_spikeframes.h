// What bq_spikeframes.hip (every frame from the row's first candle) and
// bq_spikecap.hip (the sliding frame cap) share: the argument struct, the flag
// bits of one row of a frame (spike_eval), apply_cooldown's verdict on a frame's
// last row (spike_cooldown_keeps) and the host checks of the two entries. The
// <false> instantiations are the uncapped kernels' code, unchanged by the cap
// (make isa-digest of bq_spikeframes.hip). Internal to the library.
#pragma once
#include "bq_replay.h"
#include "binquant_amd.h"

namespace bq {

constexpr int SF_QNT = 2 * WAVE;   // the quantile kernel: one wave per column

struct SpikeFramesArgs {
  const double* in[BQ_NUM_SPIKE_FRAMES_IN];
  const uint8_t* in_b[BQ_NUM_SPIKE_FRAMES_IN_B];
  const int64_t *lens, *first, *from;
  int64_t ld_in, ld_b, ld_out, S;
  int T, aligned, cap, omask;
  bq_spike_frames_params p;
  double *qv, *qp;   // workspace: the raw prefix quantiles [S][T]
  int* first_obs;    // workspace: [S][2] the first observed candle of each column (T: none)
  double *vcmr, *pbbt;
  uint8_t* out_b[BQ_NUM_SPIKE_FRAMES_OUT];
};

enum { SF_VCF = 1, SF_PBF = 2, SF_CUM = 4, SF_CUMS = 8, SF_PRE = 16, SF_SPRE = 32, SF_ACC = 64, SF_ACCS = 128 };

// the row's input columns, offset so that [u] is candle u of the panel
struct SpikeFramesRow {
  const double *vr, *pca, *dyn, *bsp, *cp, *cn, *op, *cl;
  const uint8_t *acc, *accs;
  int first;
};

// A capped frame [f, t] of a row (CAP): f = max(first, t + 1 - frame_cap) and g, its first valid close at or
// after f. price_change has no pad-filled source inside the frame on rows <= g.
struct SpikeFrame {
  int f, g;
};

// the capped call's further columns, offset like the row's others; shift: the offset of their VALUES (candles)
struct SpikeCapRow : SpikeFramesRow {
  const int32_t *dsrc, *cnext;
  int shift;
};

constexpr int SF_DYN_W = 60, SF_DYN_MIN = 20;   // rolling(60, min_periods=20).quantile(q) (:376-378)

// That rolling quantile at a row whose window is cut at the frame's first price change: pandas' roll_quantile
// ('linear') of rows a .. b of x, b - a < 59. Per lane, rank selection by counting: at most 59 x 59 compares on
// values the walk has in L1. +-inf is missing (win_ok), as in every pandas window.
__device__ __forceinline__ double spike_zone_quantile(const double* __restrict__ x, int a, int b, double q) {
  int n = 0;
  for (int j = a; j <= b; ++j) n += win_ok(x[j]) ? 1 : 0;
  if (n < SF_DYN_MIN) return qnan();
  const double idxf = q * (double)(n - 1);
  const int idx = (int)idxf;
  double lo = qnan(), hi = qnan();
  for (int j = a; j <= b; ++j) {
    const double xj = x[j];
    if (!win_ok(xj)) continue;
    int r = 0;
    for (int i = a; i <= b; ++i) {
      const double xi = x[i];
      r += (win_ok(xi) && (xi < xj || (xi == xj && i < j))) ? 1 : 0;
    }
    if (r == idx) lo = xj;
    if (r == idx + 1) hi = xj;
  }
  return (double)idx == idxf ? lo : lo + (hi - lo) * (idxf - (double)idx);
}

// A walk's frame is wave-uniform, so its cut window's values are too: rows g + 1 .. g + 59, sorted once per
// walk by the whole wave. Lane s holds the s-th smallest observation (val) and its row's offset from g + 1
// (off), the rows without one after them; ok: bit j = row g + 1 + j of the frame holds an observation.
struct SpikeZone {
  double val;
  int off;
  uint64_t ok;
};

__device__ __forceinline__ SpikeZone spike_zone_sort(const double* __restrict__ x, int g, int tend, int lane) {
  const int r = g + 1 + lane;
  const bool have = lane < SF_DYN_W - 1 && r <= tend;
  const double v = have ? x[r] : qnan();
  const bool ok = have && win_ok(v);
  const uint64_t okm = __ballot(ok);
  int rank = 0;   // a bijection of the lanes: the observations by (value, lane), then the other lanes
  for (int i = 0; i < WAVE; ++i) {
    const double vi = readlane_f64(v, i);
    const bool oki = (okm >> i) & 1ull;
    const bool before = ok ? oki && (vi < v || (vi == v && i < lane)) : oki || i < lane;
    rank += before ? 1 : 0;
  }
  SpikeZone Z;
  Z.val = __hiloint2double(__builtin_amdgcn_ds_permute(rank << 2, __double2hiint(v)),
                           __builtin_amdgcn_ds_permute(rank << 2, __double2loint(v)));
  Z.off = __builtin_amdgcn_ds_permute(rank << 2, lane);
  Z.ok = okm;
  asm volatile("" : "+v"(Z.ok));
  return Z;
}

// spike_zone_quantile of rows g + 1 .. g + m from the walk's sorted values: the same two order statistics,
// found by one pass over the sorted lanes (wave-uniform trip count, per-lane m).
__device__ __forceinline__ double spike_zone_pick(const SpikeZone& Z, int m, double q) {
  if (m < 1) return qnan();
  const int n = __popcll(Z.ok & ((1ull << m) - 1ull));   // m <= 59
  if (n < SF_DYN_MIN) return qnan();
  const double idxf = q * (double)(n - 1);
  const int idx = (int)idxf;
  const int nall = __popcll(Z.ok);
  int c = 0;
  double lo = qnan(), hi = qnan();
  for (int s = 0; s < nall; ++s) {
    const double vs = readlane_f64(Z.val, s);
    const int os = __builtin_amdgcn_readlane(Z.off, s);
    if (os < m) {
      if (c == idx) lo = vs;
      if (c == idx + 1) hi = vs;
      ++c;
    }
  }
  return (double)idx == idxf ? lo : lo + (hi - lo) * (idxf - (double)idx);
}

// before a walk evaluates the 64 rows from u0 on: sort the zone's values if the block can reach them
template <class Row>
__device__ __forceinline__ void spike_zone_prepare(const Row& P, SpikeFrame F, int tend, int u0, int lane,
                                                   SpikeZone& Z, bool& ready) {
  if (!ready && F.f > P.first && u0 < F.g + SF_DYN_W) {   // wave-uniform
    Z = spike_zone_sort(P.pca, F.g, tend, lane);
    ready = true;
  }
}

// The flag bits of row u of the frame [first, tend] under (vc, pb)
// (apply_preliminary_label, :350-488); 0 outside the frame. CAP: of the frame [F.f, tend], whose columns near its
// start are frame-local (bq_spike_frames_capped's rule table); the two acceleration flags come back as bits too.
template <bool CAP = false, class Row, class K>
__device__ __forceinline__ unsigned spike_eval(const Row& P, K k, int u, int tend, double vc, double pb,
                                               SpikeFrame F = SpikeFrame{0, 0}, SpikeZone Z = SpikeZone{0.0, 0, 0ull},
                                               bool sorted = false) {
  int lo = P.first, vlo = P.first;   // the frame's first row; the first row that has a volume_ratio in it
  if constexpr (CAP) {
    lo = F.f;
    vlo = F.f + k->c.base_window - 1;
  }
  if (u < lo || u > tend) return 0u;
  const int vw = k->p.volume_cluster_window, mc = k->p.volume_cluster_min_count;
  const int cw = k->p.cumulative_price_window, mode = k->p.label_mode;
  const double vc8 = vc * 0.8;
  // bit j: volume_ratio >= vc (m) / >= 0.8 vc (m8) at candle u + 1 - j; a candle outside the frame has no bit
  const int nb = vw + 2 > cw + 1 ? vw + 2 : cw + 1;   // <= 32
  unsigned m = 0u, m8 = 0u;
  for (int j = 0; j < nb; ++j) {
    const int w = u + 1 - j;
    if (w >= vlo && w <= tend) {
      const double x = P.vr[w];
      m |= (x >= vc ? 1u : 0u) << j;
      m8 |= (x >= vc8 ? 1u : 0u) << j;
    }
  }
  // rolling(vw, min_periods=1).sum() >= mc, and the row's own condition (:351-353)
  const unsigned wmask = (1u << vw) - 1u;
  const bool base_n = (m & 1u) && __popc(m & wmask) >= mc;                  // row u + 1 (none at u == tend)
  const bool base_u = ((m >> 1) & 1u) && __popc((m >> 1) & wmask) >= mc;
  const bool base_p = ((m >> 2) & 1u) && __popc((m >> 2) & wmask) >= mc;    // row u - 1
  const bool vcf = mode == 0 ? base_u && !base_n : mode == 1 ? base_u && !base_p : base_u;
  // max(pb, dyn).ffill() == max(pb, ffill(dyn)); NaN until the quantile's first value (:395-399)
  double d = P.dyn[u];
  bool pok = true, aok = true;   // the row has a price change / an acceleration operand in the frame
  if constexpr (CAP) {
    // a fill whose source row's window reaches back past g: the cut window's quantile instead (rows g + 1 ..)
    // (sorted: Z holds a walk's sorted values; a frame's newest row, whose g is its lane's own, selects by itself)
    if (F.f > P.first && P.dsrc[u] + P.shift < F.g + SF_DYN_W) {
      const int last = u < F.g + SF_DYN_W - 1 ? u : F.g + SF_DYN_W - 1;
      const double q = k->c.price_break_dynamic_q;
      d = sorted ? spike_zone_pick(Z, last - F.g, q) : spike_zone_quantile(P.pca, F.g + 1, last, q);
    }
    pok = u > F.g;
    aok = pok && u - k->c.accel_volume_deriv_window >= vlo;
  }
  const bool pbf = d == d && pok && P.pca[u] >= (pb > d ? pb : d);
  // (volume_ratio >= 0.8 vc).rolling(cw).max().astype(bool): NaN -> True on the first cw - 1 rows (:412-417)
  const bool volc = u - lo < cw - 1 || ((m8 >> 1) & ((1u << cw) - 1u)) != 0u;
  const double cth = k->p.cumulative_price_threshold;
  bool cum = P.cp[u] >= cth && volc, cums = P.cn[u] >= cth && volc;
  if constexpr (CAP) {
    if (u - cw < F.g) cum = cums = false;   // the clip sums' window holds a row <= g
  }
  const bool combo = k->p.require_both_patterns ? vcf && pbf : vcf || pbf;
  const double o = P.op[u], c = P.cl[u];
  const double bmin = k->p.body_size_pct_min;
  const bool big = bmin > 0.0 ? P.bsp[u] >= bmin : true;
  const bool pre = (combo || cum || (aok && P.acc[u] != 0)) && (!k->p.require_bullish_spike || c > o) && big;
  const bool spre = (combo || cums || (aok && P.accs[u] != 0)) && c < o && big;
  unsigned bits = (vcf ? SF_VCF : 0) | (pbf ? SF_PBF : 0) | (cum ? SF_CUM : 0) | (cums ? SF_CUMS : 0) |
                  (pre ? SF_PRE : 0) | (spre ? SF_SPRE : 0);
  if constexpr (CAP) bits |= !aok ? 0 : (P.acc[u] != 0 ? SF_ACC : 0) | (P.accs[u] != 0 ? SF_ACCS : 0);
  return bits;
}

// apply_cooldown on the frame [first, t] under (vc, pb), for its last row, whose
// label bit `side` is set: kept or not. Wave-uniform arguments and result. CAP: on the frame [F.f, t].
template <bool CAP = false, class Row, class K>
__device__ __forceinline__ bool spike_cooldown_keeps(const Row& P, K k, int t, double vc, double pb, unsigned side,
                                                     int bars, int lane, SpikeFrame F = SpikeFrame{0, 0}) {
  const int first = CAP ? F.f : P.first;
  const int ub0 = t - (WAVE - 1);
  SpikeZone Z{0.0, 0, 0ull};
  bool zready = false;
  if constexpr (CAP) {
    asm volatile("" : "+v"(vc), "+v"(pb));   // the walk's uniform state fills the SGPR file: the thresholds in VGPRs
    spike_zone_prepare(P, F, t, ub0, lane, Z, zready);
  }
  const uint64_t M0 =
      __ballot((spike_eval<CAP>(P, k, ub0 + lane, t, vc, pb, F, Z, zready) & side) != 0u);   // bit 63: row t
  // back from t - 1 to the nearest run of `bars` clear rows (rows before the frame are clear)
  uint64_t cur = M0;
  int ub = ub0, pos = WAVE - 1, clean = 0, start = first;
  bool found = false;
  for (;;) {
    for (;;) {
      const uint64_t sub = pos >= 64 ? cur : cur & ((1ull << pos) - 1ull);
      const int hi = sub ? 63 - __builtin_clzll(sub) : -1;
      const int zeros = pos - 1 - hi;
      if (clean + zeros >= bars) {
        start = ub + hi + 1;
        found = true;
        break;
      }
      if (hi < 0) {
        clean += zeros;
        break;
      }
      clean = 0;
      pos = hi;
    }
    if (found || ub <= first) break;
    ub -= WAVE;
    pos = WAVE;
    if constexpr (CAP) spike_zone_prepare(P, F, t, ub, lane, Z, zready);
    cur = __ballot((spike_eval<CAP>(P, k, ub + lane, t, vc, pb, F, Z, zready) & side) != 0u);
  }
  if (!found || start < first) start = first;
  // the greedy rule forward from `start` (:506-518)
  int last = -0x40000000;
  if (start >= ub0) {   // inside the first block: its mask is at hand
    uint64_t m = M0 & (~0ull << (start - ub0));
    while (m) {
      const int i = __builtin_ctzll(m);
      m &= m - 1;
      if (ub0 + i - last > bars) last = ub0 + i;
    }
  } else {
    for (int fb = start; fb <= t; fb += WAVE) {
      if constexpr (CAP) spike_zone_prepare(P, F, t, fb, lane, Z, zready);
      uint64_t m = __ballot((spike_eval<CAP>(P, k, fb + lane, t, vc, pb, F, Z, zready) & side) != 0u);
      while (m) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        if (fb + i - last > bars) last = fb + i;
      }
    }
  }
  return last == t;
}

// ---- host side ----------------------------------------------------------------
// the checks and fields the two entries share; BQ_OK with `run` false: nothing to launch
inline int spike_frames_setup(SpikeFramesArgs& A, const double* const* in, int64_t ld_in, const uint8_t* const* in_b,
                       int64_t ld_b, int32_t aligned, const int64_t* lens, const int64_t* first_t,
                       const int64_t* from_t, int64_t S, int64_t T, int64_t max_T,
                       const bq_spike_frames_params* params, double* vcmr, double* pbbt, uint8_t* const* out_b,
                       int64_t ld_out) {
  if (!in || !in_b || S < 0 || T < 0 || ld_in < T || ld_b < T || ld_out < T || T > max_T) return BQ_EINVAL;
  for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_IN; ++j)
    if (!(A.in[j] = in[j])) return BQ_EINVAL;
  for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_IN_B; ++j)
    if (!(A.in_b[j] = in_b[j])) return BQ_EINVAL;
  if (params) A.p = *params;
  else bq_spike_frames_default_params(&A.p);
  const bq_spike_frames_params& p = A.p;
  if (p.volume_cluster_window < 1 || p.volume_cluster_window > BQ_SPIKE_FRAMES_MAX_WINDOW ||
      p.cumulative_price_window < 2 || p.cumulative_price_window > BQ_SPIKE_FRAMES_MAX_WINDOW ||
      p.volume_cluster_min_count < 0 || p.label_mode < 0 || p.label_mode > 2 ||
      p.post_spike_cooldown_bars >= BQ_SPIKE_FRAMES_MAX_COOLDOWN ||
      !(p.volume_quantile >= 0.0 && p.volume_quantile <= 1.0) ||
      !(p.price_base_floor_quantile >= 0.0 && p.price_base_floor_quantile <= 1.0) ||
      !all_finite({p.cumulative_price_threshold, p.body_size_pct_min, p.volume_cluster_min_ratio,
                   p.price_break_base_threshold, p.min_volume_ratio, p.min_price_abs_floor}))
    return BQ_EINVAL;
  A.omask = 0;
  for (int j = 0; j < BQ_NUM_SPIKE_FRAMES_OUT; ++j) {
    A.out_b[j] = out_b ? out_b[j] : nullptr;
    A.omask |= A.out_b[j] ? 1 << j : 0;
  }
  A.vcmr = vcmr;
  A.pbbt = pbbt;
  A.omask |= (vcmr ? 1 << BQ_NUM_SPIKE_FRAMES_OUT : 0) | (pbbt ? 1 << (BQ_NUM_SPIKE_FRAMES_OUT + 1) : 0);
  A.lens = lens;
  A.first = first_t;
  A.from = from_t;
  A.ld_in = ld_in;
  A.ld_b = ld_b;
  A.ld_out = ld_out;
  A.S = S;
  A.T = (int)T;
  A.aligned = aligned ? 1 : 0;
  return BQ_OK;
}

}  // namespace bq
