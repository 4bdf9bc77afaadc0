"""numpy / pandas restatement of FailedSpikeFade.latest_signal() on every
frame df.iloc[first:t + 1] of a row (strategies/failed_spike_fade.py:229-594),
a fresh instance per frame: what strategies.failed_spike_frames and
bq_spike_frames compute. Pinned to the real class by
tests/golden/spikeframes.npz (tests/test_spikeframes_ref.py).

Two facts carry it (both checked against the fixture):

* only auto_calibrate's two scalars are frame-wide. Every other column that
  detect() reads is causal: its value at row u is the same in every frame that
  holds u (frame_columns, formed once per row with pandas' own rolling
  kernels). Under a frame's thresholds (vc, pb) the labels of its rows are
  element-wise in those columns, looking 1 row ahead ('last' label mode; the
  frame's last row has no next) and up to 30 rows back.
* apply_cooldown's greedy walk can start at any run of `bars` rows without a
  preliminary label: the first label after such a run is kept whatever
  happened before it. frames() walks from the frame's first row, as the class
  does; frames(back_walk=True) walks back from t to the nearest such run.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd

BOOL_KEYS = ("label", "label_pre", "label_short", "label_short_pre", "volume_cluster_flag", "price_break_flag",
             "cumulative_price_break_flag", "cumulative_price_break_short_flag", "accel_spike_flag",
             "accel_spike_short_flag", "upward", "downward")
FLOAT_KEYS = ("volume_cluster_min_ratio", "price_break_base_threshold", "close_open_ratio")
KEYS = BOOL_KEYS + FLOAT_KEYS


@dataclass
class Params:
    """FailedSpikeFade's attributes (:66-91) and auto_calibrate's defaults (:229-235)."""

    volume_cluster_min_ratio: float = 1.6
    volume_cluster_window: int = 8
    volume_cluster_min_count: int = 2
    volume_cluster_label_mode: str = "last"
    price_break_base_threshold: float = 0.03
    price_break_dynamic_q: float = 0.85
    cumulative_price_window: int = 3
    cumulative_price_threshold: float = 0.025
    accel_volume_deriv_window: int = 3
    accel_volume_deriv_min: float = 0.45
    accel_price_change_min: float = 0.015
    require_both_patterns: bool = False
    post_spike_cooldown_bars: int = 8
    require_bullish_spike: bool = True
    body_size_pct_min: float = 0.005
    base_window: int = 12
    streak_length: int = 3
    volume_quantile: float = 0.97
    price_base_floor_quantile: float = 0.75
    min_volume_ratio: float = 1.15
    min_price_abs_floor: float = 0.015


def frame_columns(o, c, v, p: Params) -> dict[str, np.ndarray]:
    """The threshold-independent columns of one frame (1-D arrays, row 0 the frame's first)."""
    o, c, v = (pd.Series(np.asarray(x, np.float64)) for x in (o, c, v))
    cf = c.ffill()
    pc = cf / cf.shift(1) - 1           # pct_change(): fill_method='pad'
    pca = pc.abs()
    vr = v / (v.rolling(p.base_window).mean() + 1e-6)
    vd = vr - vr.shift(p.accel_volume_deriv_window)
    acc = (vd >= p.accel_volume_deriv_min) & (pca >= p.accel_price_change_min)
    n = p.streak_length
    return dict(
        volume_ratio=vr.to_numpy(), price_change_abs=pca.to_numpy(),
        dyn=pca.rolling(60, min_periods=20).quantile(p.price_break_dynamic_q).ffill().to_numpy(),
        body_size_pct=((c - o).abs() / (o + 1e-6)).to_numpy(), bull=(c > o).to_numpy(), bear=(c < o).to_numpy(),
        cum_pos=pc.clip(lower=0).rolling(p.cumulative_price_window).sum().to_numpy(),
        cum_neg=pc.clip(upper=0).abs().rolling(p.cumulative_price_window).sum().to_numpy(),
        accel=(acc & (pc > 0)).to_numpy(), accel_short=(acc & (pc < 0)).to_numpy(),
        close_open_ratio=((c - o) / (o + 1e-6)).to_numpy(),
        upward=((c > o).astype(int).rolling(n).sum() >= n).to_numpy(),
        downward=((c < o).astype(int).rolling(n).sum() >= n).to_numpy())


def thresholds(cols, t: int, p: Params) -> tuple[float, float]:
    """auto_calibrate on the frame's rows 0 .. t (:229-257), a fresh instance."""
    vols, pcs = cols["volume_ratio"][:t + 1], cols["price_change_abs"][:t + 1]
    vols, pcs = vols[~np.isnan(vols)], pcs[~np.isnan(pcs)]
    if len(vols) == 0 or len(pcs) == 0:
        return p.volume_cluster_min_ratio, p.price_break_base_threshold
    vc = float(max(p.min_volume_ratio, np.quantile(vols, p.volume_quantile)))
    floor = float(max(p.min_price_abs_floor, np.quantile(pcs, p.price_base_floor_quantile)))
    return vc, max(p.price_break_base_threshold, floor)


def flags_under(cols, vc: float, pb: float, t: int, p: Params) -> dict[str, np.ndarray]:
    """apply_preliminary_label's columns (:350-488) on the frame's rows 0 .. t under (vc, pb)."""
    n = t + 1
    vr, pca = cols["volume_ratio"][:n], cols["price_change_abs"][:n]
    with np.errstate(invalid="ignore"):
        cond = vr >= vc
        cond8 = vr >= vc * 0.8
        cs = np.r_[0, np.cumsum(cond)]
        lo = np.maximum(np.arange(n) + 1 - p.volume_cluster_window, 0)
        base = ((cs[1:] - cs[lo]) >= p.volume_cluster_min_count) & cond
        if p.volume_cluster_label_mode == "last":
            vcf = base & ~np.r_[base[1:], False]
        elif p.volume_cluster_label_mode == "first":
            vcf = base & ~np.r_[False, base[:-1]]
        else:
            vcf = base
        pbf = pca >= np.maximum(pb, cols["dyn"][:n])
        w = p.cumulative_price_window
        c8 = np.r_[0, np.cumsum(cond8)]
        vol_cond = np.arange(n) < w - 1                      # rolling(w).max() is NaN there: astype(bool) -> True
        vol_cond = vol_cond | ((c8[1:] - c8[np.maximum(np.arange(n) + 1 - w, 0)]) > 0)
        cum = (cols["cum_pos"][:n] >= p.cumulative_price_threshold) & vol_cond
        cum_s = (cols["cum_neg"][:n] >= p.cumulative_price_threshold) & vol_cond
        combo = (vcf & pbf) if p.require_both_patterns else (vcf | pbf)
        pre = combo | cum | cols["accel"][:n]
        if p.require_bullish_spike:
            pre = pre & cols["bull"][:n]
        spre = (combo | cum_s | cols["accel_short"][:n]) & cols["bear"][:n]
        if p.body_size_pct_min > 0:
            big = cols["body_size_pct"][:n] >= p.body_size_pct_min
            pre, spre = pre & big, spre & big
    return dict(volume_cluster_flag=vcf, price_break_flag=pbf, cumulative_price_break_flag=cum,
                cumulative_price_break_short_flag=cum_s, label_pre=pre, label_short_pre=spre)


def kept_last(pre: np.ndarray, bars: int, start: int = 0) -> bool:
    """apply_cooldown's greedy walk (:495-520) from row `start`: is the last row's label kept?"""
    if bars <= 0:
        return bool(pre[-1])
    last, kept = None, False
    for i in range(start, len(pre)):
        if pre[i]:
            kept = not (last is not None and i - last <= bars)
            if kept:
                last = i
    return bool(pre[-1]) and kept


def walk_start(pre: np.ndarray, bars: int) -> int:
    """From the last row back to the nearest run of `bars` rows without a label: the run's first row, or 0."""
    u, clean = len(pre) - 2, 0
    while u >= 0 and clean < bars:
        clean = 0 if pre[u] else clean + 1
        u -= 1
    return u + 1


def frames_row(o, c, v, p: Params | None = None, back_walk: bool = False, walks: list | None = None):
    """One row's frame (1-D arrays from its first candle to its last):
    {key: array over t} of KEYS. walks: receives the back-walk lengths."""
    p = p or Params()
    cols = frame_columns(o, c, v, p)
    n = len(cols["volume_ratio"])
    out = {k: np.zeros(n, bool) for k in BOOL_KEYS}
    out.update({k: np.full(n, np.nan) for k in FLOAT_KEYS})
    bars = p.post_spike_cooldown_bars
    for t in range(n):
        vc, pb = thresholds(cols, t, p)
        f = flags_under(cols, vc, pb, t, p)
        out["volume_cluster_min_ratio"][t], out["price_break_base_threshold"][t] = vc, pb
        for k, x in f.items():
            out[k][t] = x[t]
        for k, kp in (("label", "label_pre"), ("label_short", "label_short_pre")):
            pre = f[kp]
            if not pre[t]:
                continue
            start = 0
            if back_walk and bars > 0:
                start = walk_start(pre, bars)
                if walks is not None:
                    walks.append(t - start)
            out[k][t] = kept_last(pre, bars, start)
    for k in ("accel", "accel_short"):
        out[f"{k.replace('accel', 'accel_spike')}_flag"] = cols[k].copy()
    for k in ("upward", "downward", "close_open_ratio"):
        out[k] = cols[k].copy()
    return out


def frames(o, c, v, p: Params | None = None, first_t=None, lens=None, back_walk: bool = False,
           walks: list | None = None) -> dict[str, np.ndarray]:
    """[S, T] panels -> {key: [S, T]}; cells outside [first_t, lens) hold False / NaN."""
    S, T = np.shape(c)
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t)
    lens = np.full(S, T, np.int64) if lens is None else np.asarray(lens)
    out = {k: np.zeros((S, T), bool) for k in BOOL_KEYS}
    out.update({k: np.full((S, T), np.nan) for k in FLOAT_KEYS})
    for s in range(S):
        a, b = int(first[s]), int(lens[s])
        if b <= a:
            continue
        r = frames_row(o[s, a:b], c[s, a:b], v[s, a:b], p, back_walk, walks)
        for k in KEYS:
            out[k][s, a:b] = r[k]
    return out


SOURCE_REASONS = ("symbol_confirmed_upward_price_impulse", "symbol_price_impulse_missing",
                  "symbol_spike_too_extended", "symbol_upward_spike_missing")


def source_allows(d, max_candle_return: float = 0.06):
    """source_spike_allows (:190-203) on frames()'s dict: (ok, reason code), the first failing check."""
    impulse = d["price_break_flag"] | d["cumulative_price_break_flag"] | d["accel_spike_flag"]
    with np.errstate(invalid="ignore"):
        reason = np.where(~d["label"] | ~impulse, 1, np.where(d["close_open_ratio"] > max_candle_return, 2,
                                                             np.where(~d["upward"], 3, 0))).astype(np.uint8)
    return reason == 0, reason
