"""numpy / pandas restatement of FailedSpikeFade.latest_signal() under a
SLIDING frame cap: column t of a row = the method on a fresh instance whose
frame is df.iloc[f:t + 1], f = max(first, t + 1 - frame_cap) — what
strategies.failed_spike_frames(frame_cap=M) and bq_spike_frames_capped
compute. Pinned to the real class by tests/golden/spikecap.npz
(tests/test_spikecap_ref.py).

capped_row is the oracle: every frame is cut out of the row and handed to
tests/spikeframes_ref's functions (frames_row's own steps, for the frame's
last row only; test_spikecap_ref checks a sample against frames_row itself).

capped_row_fast mirrors the kernels: one set of columns per row, formed from
the row's first candle (spikeframes_ref.frame_columns), and per frame
  * g = the frame's first valid close at or after f: price_change is NaN on
    rows <= g (the pad fill has no source inside the frame), so the clip sums
    are NaN on rows < g + cw + 1 and price_change_abs is an observation of the
    calibration from row g + 1 on;
  * volume_ratio is NaN before f + base_window - 1 (so is the cluster count's
    and vol_cond's operand; the acceleration flag needs it aw rows back);
  * vol_cond is True on rows < f + cw - 1;
  * the rolling(60, min_periods=20) quantile of price_change_abs is the row's
    own where its window lies past g (rows >= g + 60); before that it is the
    quantile of rows g + 1 .. min(u, g + 59), NaN below 20 observations, and a
    forward fill whose source row lies before g + 60 takes that value.
Rows deeper in the frame hold the row's columns up to pandas' running-sum
rounding (pandas adds and removes from the frame's first row).

capped_row_fast(shortcut=True) is what a cheaper design would give (sliding thresholds,
the row's columns as they are, the walk stopped at f): the fixture counts the
cells where it is wrong."""

from __future__ import annotations

import numpy as np

import spikeframes_ref as sf
from spikeframes_ref import BOOL_KEYS, FLOAT_KEYS, KEYS, Params

ROW_KEYS = ("accel_spike_flag", "accel_spike_short_flag", "upward", "downward", "close_open_ratio")
ROW_COLS = ("accel", "accel_short", "upward", "downward", "close_open_ratio")
DYN_WINDOW, DYN_MIN = 60, 20


def frame_start(t: int, cap: int | None, first: int = 0) -> int:
    return first if cap is None else max(first, t + 1 - cap)


def frame_last(o, c, v, p: Params, walks: list | None = None) -> dict:
    """frames_row's last cell: one frame (1-D arrays, the whole of it) -> {key: scalar}."""
    cols = sf.frame_columns(o, c, v, p)
    t = len(cols["volume_ratio"]) - 1
    vc, pb = sf.thresholds(cols, t, p)
    f = sf.flags_under(cols, vc, pb, t, p)
    out = {k: bool(x[t]) for k, x in f.items()}
    out["volume_cluster_min_ratio"], out["price_break_base_threshold"] = vc, pb
    bars = p.post_spike_cooldown_bars
    for k, kp in (("label", "label_pre"), ("label_short", "label_short_pre")):
        out[k] = bool(f[kp][t]) and sf.kept_last(f[kp], bars)
        if walks is not None and k == "label" and f[kp][t] and bars > 0:
            walks.append(t - sf.walk_start(f[kp], bars))
    for k, kc in zip(ROW_KEYS, ROW_COLS):
        out[k] = cols[kc][t]
    return out


def _empty(n: int) -> dict[str, np.ndarray]:
    out = {k: np.zeros(n, bool) for k in BOOL_KEYS}
    out.update({k: np.full(n, np.nan) for k in FLOAT_KEYS})
    return out


def capped_row(o, c, v, cap: int | None, p: Params | None = None, from_t: int = 0, ends=None) -> dict:
    """The oracle. One row (1-D arrays from its first candle): {key: array over t}; ends: only these t.
    Frames that have not slid yet (t < cap) all start on the row's first candle: those cells are one
    frames_row call on the first `cap` candles, every later cell is a frame of its own."""
    p = p or Params()
    o, c, v = (np.asarray(x, np.float64) for x in (o, c, v))
    n = len(c)
    out = _empty(n)
    head = n if cap is None else min(cap, n)
    if ends is None and from_t < head:
        r = sf.frames_row(o[:head], c[:head], v[:head], p)
        for k in KEYS:
            out[k][from_t:head] = r[k][from_t:]
    for t in (range(max(from_t, head), n) if ends is None else ends):
        f = frame_start(t, cap)
        r = frame_last(o[f:t + 1], c[f:t + 1], v[f:t + 1], p)
        for k in KEYS:
            out[k][t] = r[k]
    return out


def _pandas_quantile(x: np.ndarray, q: float) -> float:
    """roll_quantile's 'linear' interpolation on the finite values of x (pandas/_libs/window/aggregations.pyx)."""
    x = np.sort(x[np.isfinite(x)])
    if len(x) < DYN_MIN:
        return np.nan
    idxf = q * (len(x) - 1)
    i = int(idxf)
    return float(x[i]) if i == idxf else float(x[i] + (x[i + 1] - x[i]) * (idxf - i))


def row_columns(o, c, v, p: Params) -> dict[str, np.ndarray]:
    """frame_columns of the whole row plus what the capped kernels read beside them: dyn_src[u], the row of
    the forward-filled quantile's source (-1: none), and close_next[u], the first valid close at or after u."""
    import pandas as pd

    cols = sf.frame_columns(o, c, v, p)
    n = len(cols["volume_ratio"])
    pca = pd.Series(cols["price_change_abs"])
    raw = pca.rolling(DYN_WINDOW, min_periods=DYN_MIN).quantile(p.price_break_dynamic_q).to_numpy()
    cols["dyn_src"] = np.maximum.accumulate(np.where(np.isnan(raw), -1, np.arange(n)))
    ok = ~np.isnan(np.asarray(c, np.float64))
    cols["close_next"] = np.minimum.accumulate(np.where(ok, np.arange(n), n)[::-1])[::-1]
    return cols


def local_flags(cols, f: int, t: int, vc: float, pb: float, p: Params, local: bool = True) -> tuple[dict, dict]:
    """The frame [f, t]'s label columns under (vc, pb) from the ROW's columns (arrays over u = f .. t), and
    the frame-local columns they were formed from."""
    n = t + 1 - f
    u = np.arange(f, t + 1)
    g = int(cols["close_next"][f]) if local else f - (1 << 30)
    cw, bw, aw = p.cumulative_price_window, p.base_window, p.accel_volume_deriv_window
    vr = cols["volume_ratio"][f:t + 1].copy()
    pca = cols["price_change_abs"][f:t + 1].copy()
    dyn = cols["dyn"][f:t + 1].copy()
    cp, cn = cols["cum_pos"][f:t + 1].copy(), cols["cum_neg"][f:t + 1].copy()
    acc, accs = cols["accel"][f:t + 1].copy(), cols["accel_short"][f:t + 1].copy()
    if local:
        vr[u < f + bw - 1] = np.nan
        pca[u <= g] = np.nan
        cp[u < g + cw] = np.nan
        cn[u < g + cw] = np.nan
        bad = (u - aw < f + bw - 1) | (u <= g)
        acc[bad], accs[bad] = False, False
        zone = cols["dyn_src"][f:t + 1] < g + DYN_WINDOW
        for i in np.nonzero(zone)[0]:
            hi = min(f + i, g + DYN_WINDOW - 1)
            dyn[i] = _pandas_quantile(cols["price_change_abs"][g + 1:hi + 1], p.price_break_dynamic_q) \
                if hi > g else np.nan
    sub = dict(volume_ratio=vr, price_change_abs=pca, dyn=dyn, cum_pos=cp, cum_neg=cn, accel=acc, accel_short=accs,
               bull=cols["bull"][f:t + 1], bear=cols["bear"][f:t + 1], body_size_pct=cols["body_size_pct"][f:t + 1])
    return sf.flags_under(sub, vc, pb, n - 1, p), sub


def _thresholds(cols, f: int, t: int, p: Params):
    g = int(cols["close_next"][f])
    vr = cols["volume_ratio"][min(f + p.base_window - 1, t + 1):t + 1]
    pcs = cols["price_change_abs"][min(g + 1, t + 1):t + 1]
    return sf.thresholds(dict(volume_ratio=vr, price_change_abs=pcs), t, p)


def capped_row_fast(o, c, v, cap: int | None, p: Params | None = None, shortcut: bool = False,
                    zone_walks: list | None = None) -> dict:
    """The kernels' arithmetic (shortcut=False) or the cheaper design the fixture argues against (True)."""
    p = p or Params()
    cols = row_columns(o, c, v, p)
    n = len(cols["volume_ratio"])
    out = _empty(n)
    bars = p.post_spike_cooldown_bars
    for t in range(n):
        f = frame_start(t, cap)
        g = int(cols["close_next"][f])
        vc, pb = _thresholds(cols, f, t, p)
        fl, sub = local_flags(cols, f, t, vc, pb, p, local=not shortcut)
        out["volume_cluster_min_ratio"][t], out["price_break_base_threshold"][t] = vc, pb
        for k, x in fl.items():
            out[k][t] = x[-1]
        for k, kp in (("label", "label_pre"), ("label_short", "label_short_pre")):
            pre = fl[kp]
            if pre[-1]:
                start = sf.walk_start(pre, bars) if bars > 0 else 0
                out[k][t] = sf.kept_last(pre, bars, start)
                if zone_walks is not None and f > 0 and bars > 0 and f + start <= g + DYN_WINDOW - 1:
                    zone_walks.append((t, f + start))
        out["accel_spike_flag"][t], out["accel_spike_short_flag"][t] = sub["accel"][-1], sub["accel_short"][-1]
        full = t - f >= p.streak_length - 1
        out["upward"][t], out["downward"][t] = full and cols["upward"][t], full and cols["downward"][t]
        out["close_open_ratio"][t] = cols["close_open_ratio"][t]
    return out


def frames(o, c, v, cap: int | None, p: Params | None = None, first_t=None, lens=None, from_t=None, fast=False,
           **kw) -> dict[str, np.ndarray]:
    """[S, T] panels -> {key: [S, T]}; cells outside [max(first_t, from_t), lens) hold False / NaN
    (close_open_ratio: wherever the candle is)."""
    S, T = np.shape(c)
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t)
    lens = np.full(S, T, np.int64) if lens is None else np.asarray(lens)
    frm = np.zeros(S, np.int64) if from_t is None else np.asarray(from_t)
    out = {k: np.zeros((S, T), bool) for k in BOOL_KEYS}
    out.update({k: np.full((S, T), np.nan) for k in FLOAT_KEYS})
    for s in range(S):
        a, b = int(first[s]), int(lens[s])
        if b <= a:
            continue
        lo = max(int(frm[s]) - a, 0)
        args = (o[s, a:b], c[s, a:b], v[s, a:b], cap, p)
        r = capped_row_fast(*args, **kw) if fast else capped_row(*args, from_t=lo, **kw)
        for k in KEYS:
            out[k][s, a + lo:b] = r[k][lo:]
        oo, cc = np.asarray(o[s, a:b], np.float64), np.asarray(c[s, a:b], np.float64)
        out["close_open_ratio"][s, a:b] = (cc - oo) / (oo + 1e-6)
    return out


def near_ties(o, c, v, cap: int | None, p: Params | None = None, tie: float = 1e-9) -> int:
    """The comparisons of every capped frame of a row whose sides lie within `tie` relative of each other
    without being equal (make_golden_spikeframes.near_ties' rule), from the kernels' arithmetic."""
    p = p or Params()
    cols = row_columns(o, c, v, p)

    def close(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
        ok = np.isfinite(a) & np.isfinite(b) & (a != b)
        return int((np.abs(a - b)[ok] <= tie * np.maximum(np.abs(a), np.abs(b))[ok]).sum())

    n, ties = len(cols["volume_ratio"]), 0
    for t in range(n):
        f = frame_start(t, cap)
        vc, pb = _thresholds(cols, f, t, p)
        _, sub = local_flags(cols, f, t, vc, pb, p)
        ties += close(sub["volume_ratio"], vc) + close(sub["volume_ratio"], vc * 0.8)
        ties += close(sub["price_change_abs"], np.maximum(pb, sub["dyn"]))
        ties += close(sub["cum_pos"], p.cumulative_price_threshold) + close(sub["cum_neg"], p.cumulative_price_threshold)
        ties += close(sub["body_size_pct"], p.body_size_pct_min)
    return ties
