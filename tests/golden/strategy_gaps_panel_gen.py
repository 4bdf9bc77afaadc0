"""Deterministic kline panels with missing candles for strategy_gaps.npz.

Shared by tests/golden/make_golden_strategy_gaps.py (which runs the REAL
reference functions on these rows) and the tests (which rebuild the inputs
and check the stored digest). numpy's default_rng only.

Every row is a random walk with planted bursts: a small up close, then a
+3.5 .. 6 % close on 8x volume and, four candles later, a second one (inside
the spike detector's 8-bar cooldown). The bursts lie at fixed fractions of
the row and, on gap rows, again after the row's last gap, so that the burst,
pump and spike detectors fire once their windows are clean again. Per-row
price scales cycle over 1e-2 .. 1e3; rows alternate with / without
quote_asset_volume (even rows carry it), as strategy_panel.npz does.

Short rows (T = 200), CASES in row order — "candle" = open, high, low, close
and volume all NaN:

  one_nan_close       close NaN at 100
  candle_run          candles 75..79 NaN
  late_listing        candles 0..59 NaN
  nan_volume          volume NaN at 60, 61 and 105 (quote volume with it)
  nan_tail            candles 198, 199 NaN
  empty_bins          OHLC NaN with volume 0 at 50..52 and 115 (a resample's empty bins)
  scattered_nan_high  high NaN every 33..40 candles (never 48 clean in a row)
  nan_at_zero         candle 0 NaN
  nan_open            open NaN at 90 and 91
  close_w_burst       close NaN at T-1-82: the burst score misses that candle and the next
                      (price_jump reads the previous close), and its threshold is
                      score.shift(1).rolling(80): T-1 is the first candle whose window is clean
  close_w_pump        close NaN at T-1-50: the pump score misses the candle after it (the
                      compression divides by the previous close), score.shift(1).rolling(48)
                      needs 48 values: score_threshold is NaN up to T-2 and finite at T-1
  close_w_spike       close NaN at T-1-60: the spike pass's largest window, the 60-bar
                      quantile, first leaves the candle out at T-1
  close_run_lags      close NaN at 100..105: longer than every pct_change lag (1, 3, 5)
  nan_after_spike     a burst at 110, its twin moved to 111 and candle 111 NaN: the
                      missing candle would have been labelled; a third burst at 115
                      sits inside 110's cooldown across the gap
  bench_overlap       candles 90..93 and 111 NaN against a benchmark missing
                      88..91 (overlapping) and 110 (adjacent)
  clean_a, clean_b    no gap

Long rows (T = 1100; the fused passes' 1024-candle tile edge):

  long_close_1023     close NaN at 1023
  long_run_1020       candles 1020..1030 NaN
  long_listing_1024   candles 0..1023 NaN
  long_run_halo       candles 985..1030 NaN: 46 missing candles over the tile edge, more
                      than the 32-candle halo the fused passes keep of the previous tile,
                      so the last valid close reaches the next tile only as a carry
"""

from __future__ import annotations

import hashlib

import numpy as np

FIELDS = ("open", "high", "low", "close", "volume", "quote_asset_volume")
OHLCV = ("open", "high", "low", "close", "volume")
T_SHORT, T_LONG = 200, 1100
LONG_FROM = 960            # long rows are recorded at candles LONG_FROM .. T_LONG - 1
W_BURST, W_PUMP, W_SPIKE = 80, 48, 60
SCALES = (1e-2, 3.7e-1, 1.9e1, 1e3, 6.3e-2, 4.2, 2.6e2)

SHORT_CASES = ("one_nan_close", "candle_run", "late_listing", "nan_volume", "nan_tail", "empty_bins",
               "scattered_nan_high", "nan_at_zero", "nan_open", "close_w_burst", "close_w_pump", "close_w_spike",
               "close_run_lags", "nan_after_spike", "bench_overlap", "clean_a", "clean_b")
LONG_CASES = ("long_close_1023", "long_run_1020", "long_listing_1024", "long_run_halo")
CLEAN = ("clean_a", "clean_b")
BENCH_MISSING_SHORT = (30, 31, 88, 89, 90, 91, 110, 165)
BENCH_MISSING_LONG = (300, 301, 302, 1019, 1020, 1021, 1031, 1060)


def gaps(case: str) -> dict[str, list[int]]:
    """{field: candles set NaN} of a case ('volume0': candles whose volume is 0)."""
    T = T_SHORT
    allf = lambda ts: {f: list(ts) for f in OHLCV}   # noqa: E731
    ohlc = lambda ts: {f: list(ts) for f in ("open", "high", "low", "close")}   # noqa: E731
    if case == "one_nan_close":
        return {"close": [100]}
    if case == "candle_run":
        return allf(range(75, 80))
    if case == "late_listing":
        return allf(range(0, 60))
    if case == "nan_volume":
        return {"volume": [60, 61, 105]}
    if case == "nan_tail":
        return allf([T - 2, T - 1])
    if case == "empty_bins":
        return {**ohlc([50, 51, 52, 115]), "volume0": [50, 51, 52, 115]}
    if case == "scattered_nan_high":
        g = np.random.default_rng(606)
        ts, t = [], 20
        while t < T - 3:
            ts.append(t)
            t += int(g.integers(33, 41))
        return {"high": ts}
    if case == "nan_at_zero":
        return allf([0])
    if case == "nan_open":
        return {"open": [90, 91]}
    if case == "close_w_burst":
        return {"close": [T - 1 - W_BURST - 2]}
    if case == "close_w_pump":
        return {"close": [T - 1 - W_PUMP - 2]}
    if case == "close_w_spike":
        return {"close": [T - 1 - W_SPIKE]}
    if case == "close_run_lags":
        return {"close": list(range(100, 106))}
    if case == "nan_after_spike":
        return allf([111])
    if case == "bench_overlap":
        return allf([90, 91, 92, 93, 111])
    if case == "long_close_1023":
        return {"close": [1023]}
    if case == "long_run_1020":
        return allf(range(1020, 1031))
    if case == "long_listing_1024":
        return allf(range(0, 1024))
    if case == "long_run_halo":
        return allf(range(985, 1031))
    return {}


def last_gap(case: str) -> int:
    """The last candle of the case that holds a missing value (-1: none)."""
    ts = [t for k, v in gaps(case).items() if k != "volume0" for t in v]
    return max(ts) if ts else -1


def gap_edges(case: str) -> list[int]:
    """First and last candle of every run of candles with a missing value."""
    ts = sorted({t for k, v in gaps(case).items() if k != "volume0" for t in v})
    return [t for t in ts if t - 1 not in ts or t + 1 not in ts]


def _burst_starts(case: str, T: int) -> list[int]:
    if case == "nan_after_spike":
        return [40, 80, 110, 115, 150, 180]
    lg = last_gap(case)
    starts = [int(T * f) for f in (0.16, 0.34, 0.58, 0.83)]
    if T == T_LONG:
        starts += [975, 1000, 1050]
    if 0 <= lg < T - 14:   # again once the gap is behind, and near the row's end
        starts.append(lg + 6)
        if T - 1 - lg > 40:
            starts.append(T - 8)
    return sorted({s for s in starts if 3 <= s < T - 6 and not (lg - 6 <= s <= lg + 1)})


def _row(case: str, s: int, T: int, seed: int) -> dict[str, np.ndarray]:
    g = np.random.default_rng(seed * 1000 + s)
    r = g.normal(0.0, 0.005, T)
    v = g.lognormal(3.0, 0.6, T)
    for j in _burst_starts(case, T):
        twin = j + 1 if case == "nan_after_spike" and j == 110 else j + 4
        for k in (j, twin):
            if k - 1 != j:
                r[k - 1] = 0.002
            r[k] = g.uniform(0.035, 0.06)
            v[k] *= 8.0
    c = SCALES[s % len(SCALES)] * np.exp(np.cumsum(r))
    o = np.r_[c[0], c[:-1]]
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 0.002, T))
    l = np.minimum(o, c) * (1.0 - g.uniform(0.0, 0.002, T))
    row = {"open": o, "high": h, "low": l, "close": c, "volume": v, "quote_asset_volume": v * c}
    for f, ts in gaps(case).items():
        if f == "volume0":
            row["volume"][ts] = 0.0
            row["quote_asset_volume"][ts] = 0.0
            continue
        row[f][ts] = np.nan
        if f in ("volume", "close"):
            row["quote_asset_volume"] = row["volume"] * row["close"]
    return row


def _panel(cases, T: int, seed: int, row0: int) -> dict[str, np.ndarray]:
    out = {f: np.empty((len(cases), T)) for f in FIELDS}
    for i, case in enumerate(cases):
        row = _row(case, row0 + i, T, seed)
        for f in FIELDS:
            out[f][i] = row[f]
    return out


def short_panel(seed: int = 2027) -> dict[str, np.ndarray]:
    return _panel(SHORT_CASES, T_SHORT, seed, 0)


def long_panel(seed: int = 2027) -> dict[str, np.ndarray]:
    return _panel(LONG_CASES, T_LONG, seed, len(SHORT_CASES))


def bench_series(T: int, seed: int = 2027) -> tuple[np.ndarray, np.ndarray]:
    """(keep mask, close) of the benchmark on the panel's open_time grid."""
    g = np.random.default_rng(seed + 99 + T)
    c = 60000.0 * np.exp(np.cumsum(g.normal(0.0, 0.004, T)))
    keep = np.ones(T, bool)
    keep[list(BENCH_MISSING_SHORT if T == T_SHORT else BENCH_MISSING_LONG)] = False
    return keep, c


def has_quote(row: int) -> bool:
    """Rows of the short panel, then of the long panel, counted through."""
    return row % 2 == 0


def a20_positions(case: str, T: int, lo: int = 0) -> np.ndarray:
    """Candles at which the a20 helpers are recorded: the last two and every
    candle within 25 of a gap edge (from `lo` on)."""
    ts = {T - 2, T - 1}
    for e in gap_edges(case):
        ts.update(range(max(lo, e - 25), min(T, e + 26)))
    return np.array(sorted(t for t in ts if t >= lo), dtype=np.int64)


def digest(*panels: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for p in panels:
        for f in sorted(p):
            h.update(f.encode())
            h.update(np.ascontiguousarray(p[f], dtype=np.float64).tobytes())
    return h.hexdigest()
