"""numpy / pandas restatement of RangeBbRsiMeanReversion.signal()
(strategies/range_bb_rsi_mean_reversion.py:202-274), written from the rule
table in include/binquant_amd.h, pinned to the recorded fixture
(tests/golden/rangefade_gates.npz) by test_rangefade_ref.py and used as the
oracle of the GPU tests.

features   adx / zscore of every prefix frame df.iloc[first:t + 1]: pandas'
           rolling sums, means and variances are online and causal, so one
           pass over df.iloc[first:] holds every prefix frame's last value bit
           for bit (the fixture, recorded prefix frame by prefix frame, pins
           this)
replay     the method message by message over an [S, T] panel

Point-wise arithmetic is numpy float64 in the method's operation order, which
is the Python floats' arithmetic bit for bit.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

DEFAULTS = dict(min_candles=40, adx_window=14, zscore_window=20, adx_max=32.0, long_rsi_max=35.0, short_rsi_min=65.0,
                long_zscore_max=-2.0, short_zscore_min=2.0, band_touch_tolerance=0.002, max_market_stress=0.35,
                max_symbol_atr_pct=0.04, max_symbol_bb_width=0.08, min_rejection_wick_frac=0.30,
                long_close_position_min=0.55, short_close_position_max=0.45)
REASONS = ("emit", "no_frame", "not_enough_data", "market_context_unavailable", "market_transitioning",
           "market_stress_too_high", "market_regime_unavailable", "market_regime_not_range",
           "symbol_regime_unavailable", "symbol_regime_not_range", "symbol_transition", "symbol_atr_too_high",
           "symbol_bb_width_too_high", "adx_too_high", "no_bb_rsi_rejection_setup")
(EMIT, NO_FRAME, NOT_ENOUGH_DATA, NO_CONTEXT, TRANSITIONING, STRESS, NO_REGIME, REGIME_NOT_RANGE, NO_SYMBOL,
 SYMBOL_NOT_RANGE, SYMBOL_TRANSITION, SYMBOL_ATR, SYMBOL_BB_WIDTH, ADX_TOO_HIGH, NO_SETUP) = range(15)
FEATURES = ("adx", "zscore")
VALUES = FEATURES + ("direction", "score")
CTX_ROWS = ("regime_is_transitioning", "market_stress_score", "market_regime")
MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
NONE = 255
RANGE = MARKET_REGIMES.index("RANGE")
assert MICRO_REGIMES.index("RANGE") == RANGE
BAD_TRANSITIONS = tuple(MICRO_TRANSITIONS.index(k) for k in ("BREAKOUT_UP", "BREAKDOWN", "VOLATILITY_EXPANSION"))
SYM_KEYS = ("ok", "micro_regime", "micro_transition", "atr_pct", "bb_width")
LONG, SHORT = 0.0, 1.0
TAIL = 5


def adx_series(high: pd.Series, low: pd.Series, close: pd.Series, window: int = 14) -> pd.Series:
    """The ADX of every prefix of the frame (rule table: `adx`)."""
    hd, ld = high.diff(), -low.diff()
    plus = hd.where((hd > ld) & (hd > 0), 0.0)
    minus = ld.where((ld > hd) & (ld > 0), 0.0)
    pc = close.shift(1)
    tr = pd.concat([high - low, (high - pc).abs(), (low - pc).abs()], axis=1).max(axis=1)   # skips NaN
    atr_sum = tr.rolling(window, min_periods=window).sum()
    pdi = 100.0 * plus.rolling(window, min_periods=window).sum() / atr_sum
    mdi = 100.0 * minus.rolling(window, min_periods=window).sum() / atr_sum
    tot = pdi + mdi
    dx = (100.0 * (pdi - mdi).abs() / tot.where(tot != 0, np.nan)).fillna(0.0)
    adx = dx.rolling(window, min_periods=window).mean()
    return adx.where(adx == adx, 100.0)


def zscore_series(close: pd.Series, window: int = 20) -> pd.Series:
    """The z-score of every prefix of the frame (rule table: `zscore`)."""
    mean = close.rolling(window, min_periods=window).mean()
    std = close.rolling(window, min_periods=window).std(ddof=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (close - mean) / std
    return z.where((std != 0) & (std == std), 0.0)


def features(high, low, close, first_t=None, lens=None, P=DEFAULTS) -> dict:
    S, T = close.shape
    out = {k: np.full((S, T), np.nan) for k in FEATURES}
    for s in range(S):
        f = 0 if first_t is None else int(first_t[s])
        n = T if lens is None else int(lens[s])
        if f >= n:
            continue
        h, l, c = (pd.Series(np.asarray(x[s, f:n], np.float64)) for x in (high, low, close))
        out["adx"][s, f:n] = adx_series(h, l, c, int(P["adx_window"])).to_numpy()
        out["zscore"][s, f:n] = zscore_series(c, int(P["zscore_window"])).to_numpy()
    return out


def pymax(a, b):
    """Python's max(a, b) element-wise: a unless b > a."""
    return np.where(b > a, b, a)


def pymin(a, b):
    return np.where(b < a, b, a)


def rejections(o, h, l, c, bb_upper, bb_lower, P=DEFAULTS):
    """(_bullish_rejection, _bearish_rejection) of every candle."""
    with np.errstate(invalid="ignore", divide="ignore"):
        rng = h - l
        pos = (c - l) / rng
        live = ~(rng <= 0)
        bull = live & (l <= bb_lower * (1.0 + P["band_touch_tolerance"])) & (c > o) \
            & ((pymin(o, c) - l) / rng >= P["min_rejection_wick_frac"]) & (pos >= P["long_close_position_min"])
        bear = live & (h >= bb_upper * (1.0 - P["band_touch_tolerance"])) & (c < o) \
            & ((h - pymax(o, c)) / rng >= P["min_rejection_wick_frac"]) & (pos <= P["short_close_position_max"])
    return bull, bear


def null_tail(cols, first, T):
    """A NaN in any of `cols` within the frame's last min(5, rows) candles."""
    S = cols[0].shape[0]
    t = np.arange(T)[None, :]
    nul = np.zeros((S, T), bool)
    for x in cols:
        nul |= np.isnan(x)
    nul &= t >= first[:, None]
    out = np.zeros((S, T), bool)
    for k in range(TAIL):
        out[:, k:] |= nul[:, :T - k]
    return out


def replay(o, h, l, c, v, rsi, bb_upper, bb_mid, bb_lower, ctx, ctx_ok=None, *, sym=None, features_given=None,
           first_t=None, lens=None, from_t=None, **params):
    """Column t of row s = signal() on the message whose frame is
    df.iloc[first_t[s]:t + 1]. sym: None or {SYM_KEYS: [S] or [S, T]};
    features_given: None or {FEATURES: [S, T]}. Returns status and VALUES."""
    P = {**DEFAULTS, **params}
    S, T = c.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    frm = np.zeros(S, np.int64) if from_t is None else np.clip(np.asarray(from_t, np.int64), 0, T)
    frm = np.maximum(frm, first)
    ft = features_given if features_given is not None else features(h, l, c, first, ln, P)
    adx, z = ft["adx"], ft["zscore"]
    ctx = np.broadcast_to(ctx, (3, T))
    ok = np.ones(T, bool) if ctx_ok is None else np.broadcast_to(np.asarray(ctx_ok).astype(bool), (T,))
    if sym is None:
        sy = dict(ok=np.zeros((S, T), bool), micro_regime=np.full((S, T), NONE), micro_transition=np.full((S, T), NONE),
                  atr_pct=np.zeros((S, T)), bb_width=np.zeros((S, T)))
    else:
        sy = {k: np.broadcast_to(np.asarray(sym[k])[:, None] if np.asarray(sym[k]).ndim == 1 else np.asarray(sym[k]),
                                 (S, T)) for k in SYM_KEYS}
        sy["ok"] = sy["ok"].astype(bool)
    t = np.arange(T)[None, :]
    valid = (t >= frm[:, None]) & (t < ln[:, None])
    trans, stress, regime = (np.broadcast_to(ctx[i][None, :], (S, T)) for i in range(3))
    bull, bear = rejections(o, h, l, c, bb_upper, bb_lower, P)
    with np.errstate(invalid="ignore", divide="ignore"):
        lng = (c <= bb_mid) & (rsi <= P["long_rsi_max"]) & (z <= P["long_zscore_max"]) & bull
        sht = (c >= bb_mid) & (rsi >= P["short_rsi_min"]) & (z >= P["short_zscore_min"]) & bear
        short_frame = (t + 1 - first[:, None] < P["min_candles"]) | null_tail((o, h, l, c, rsi, v), first, T)
        checks = (   # the last one that holds wins: listed in reverse order of the method
            (NO_SETUP, ~lng & ~sht),
            (ADX_TOO_HIGH, adx > P["adx_max"]),
            (SYMBOL_BB_WIDTH, sy["bb_width"] > P["max_symbol_bb_width"]),
            (SYMBOL_ATR, sy["atr_pct"] > P["max_symbol_atr_pct"]),
            (SYMBOL_TRANSITION, np.isin(sy["micro_transition"], BAD_TRANSITIONS)),
            (SYMBOL_NOT_RANGE, sy["micro_regime"] != RANGE),
            (NO_SYMBOL, ~sy["ok"]),
            (REGIME_NOT_RANGE, regime != RANGE),
            (NO_REGIME, regime == NONE),
            (STRESS, stress >= P["max_market_stress"]),
            (TRANSITIONING, trans != 0),
            (NO_CONTEXT, np.broadcast_to(~ok[None, :], (S, T))),
            (NOT_ENOUGH_DATA, short_frame),
            (NO_FRAME, ~valid))
        status = np.full((S, T), EMIT, np.uint8)
        for code, m in checks:
            status[m] = code
        # local_score, unrounded, in the method's operation order
        rpart = np.where(lng, pymax(0.0, (P["long_rsi_max"] - rsi) / P["long_rsi_max"]),
                         pymax(0.0, (rsi - P["short_rsi_min"]) / 35.0))
        score = ((1.0 + pymin(np.abs(z) / 3.0, 1.0) * 0.35) + pymax(0.0, (P["adx_max"] - adx) / P["adx_max"]) * 0.25) \
            + rpart * 0.25
    emit = status == EMIT
    out = dict(status=status)
    out["adx"] = np.where(emit | (status >= ADX_TOO_HIGH), adx, np.nan)
    out["zscore"] = np.where(emit | (status >= NO_SETUP), z, np.nan)
    out["direction"] = np.where(emit, np.where(lng, LONG, SHORT), np.nan)
    out["score"] = np.where(emit, score, np.nan)
    return out
