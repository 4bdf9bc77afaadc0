"""numpy / pandas restatement of MeanReversionFade.signal()
(strategies/mean_reversion_fade.py:224-300), pinned to the recorded fixture
(tests/golden/meanrev_gates.npz) by test_meanrev_ref.py and used as the
oracle of the GPU tests.

features   rsi / previous_rsi / volume_ma / atr_ma / trend_score of every
           prefix frame df.iloc[first:t + 1]: pandas' own ewm / rolling are
           causal, so one pass over df.iloc[first:] holds every frame's last
           values bit for bit
replay     the method message by message over an [S, T] panel

Point-wise arithmetic is numpy float64 in the method's operation order, which
is the Python floats' arithmetic bit for bit.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

DEFAULTS = dict(rsi_window=14, volume_ma_window=20, atr_ma_window=20, ema_fast=20, ema_slow=50, rsi_short_min=76.0,
                volume_ratio_min=0.8, atr_spike_max=2.2, atr_stop_mult=2.0, max_entry_stop_loss_pct=1.5,
                max_trend_score=0.005, max_market_stress=0.25, max_gap=0.02, max_symbol_atr_pct=0.03,
                min_wick_ratio=0.0)
REASONS = ("emit", "no_frame", "indicators_not_ready", "atr_volatility_spike", "volume_below_average",
           "invalid_candle_range", "no_fade_setup", "trend_score_above_max", "market_context_unavailable",
           "market_stress_too_high", "symbol_atr_too_high", "market_context_long_edge", "btc_context_up",
           "symbol_breakout_up", "symbol_trend_up", "candle_already_emitted", "entry_stop_loss_too_wide")
(EMIT, NO_FRAME, NOT_READY, ATR_SPIKE, LOW_VOLUME, BAD_RANGE, NO_SETUP, TREND_TOO_HIGH, NO_CONTEXT, STRESS,
 SYMBOL_ATR, LONG_EDGE, BTC_UP, BREAKOUT_UP, SYMBOL_TREND_UP, ALREADY_EMITTED, STOP_TOO_WIDE) = range(17)
FEATURES = ("rsi", "previous_rsi", "volume_ma", "atr_ma", "trend_score")
VALUES = FEATURES + ("stop_loss_pct", "score")
CTX_ROWS = ("market_stress_score", "long_regime_score", "short_regime_score", "btc_regime_score", "btc_return")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
NONE = 255
TREND_UP, BREAKOUT_UP_CODE = MICRO_REGIMES.index("TREND_UP"), MICRO_TRANSITIONS.index("BREAKOUT_UP")
SYM_KEYS = ("ok", "atr_pct", "trend_score", "micro_regime", "micro_transition")


def rsi_series(closes: pd.Series, window: int = 14) -> pd.Series:
    """_rsi (:88-109)."""
    delta = closes.diff()
    gain = delta.clip(lower=0)
    loss = -delta.clip(upper=0)
    avg_gain = gain.ewm(alpha=1 / window, min_periods=window, adjust=False).mean()
    avg_loss = loss.ewm(alpha=1 / window, min_periods=window, adjust=False).mean()
    denom = avg_gain + avg_loss
    return (100 * avg_gain / denom).where(denom != 0, 50.0)


def features(close, volume, atr, first_t=None, lens=None, P=DEFAULTS) -> dict:
    S, T = close.shape
    out = {k: np.full((S, T), np.nan) for k in FEATURES}
    for s in range(S):
        f = 0 if first_t is None else int(first_t[s])
        n = T if lens is None else int(lens[s])
        if f >= n:
            continue
        c = pd.Series(close[s, f:n])
        rsi = rsi_series(c, P["rsi_window"]).to_numpy()
        out["rsi"][s, f:n] = rsi
        out["previous_rsi"][s, f + 1:n] = rsi[:-1]
        out["volume_ma"][s, f:n] = pd.Series(volume[s, f:n]).rolling(P["volume_ma_window"]).mean().to_numpy()
        out["atr_ma"][s, f:n] = pd.Series(atr[s, f:n]).rolling(P["atr_ma_window"]).mean().to_numpy()
        fast = c.ewm(span=P["ema_fast"], adjust=False).mean().to_numpy()
        slow = c.ewm(span=P["ema_slow"], adjust=False).mean().to_numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            out["trend_score"][s, f:n] = np.where(slow == 0, 0.0, (fast - slow) / np.abs(slow))   # :149-155
    return out


def stop_loss_pct(atr, close, P=DEFAULTS):
    """_stop_loss_pct (:163-167) without its round_numbers."""
    with np.errstate(invalid="ignore", divide="ignore"):
        pct = (P["atr_stop_mult"] * atr / close) * 100.0
        m = np.where(0.0 > pct, 0.0, pct)       # max(pct, 0.0)
        m = np.where(101.0 < m, 101.0, m)       # min(.., 101.0)
        return np.where(close <= 0, 0.0, m)


def score(rsi, P=DEFAULTS):
    """_score (:157-161) without its round."""
    with np.errstate(invalid="ignore"):
        depth = (rsi - P["rsi_short_min"]) / (100.0 - P["rsi_short_min"])
        return 1.0 + np.where(depth > 0.0, depth, 0.0)


def gates(o, h, l, c, v, atr, bb_upper, ft, ctx, ok, sym, P=DEFAULTS):
    """The status of every cell before the once-per-candle test and the
    stop-loss cap (EMIT where the method reaches :291)."""
    S, T = c.shape
    rsi, prsi, vma, ama, trend = (ft[k] for k in FEATURES)
    stress, longr, shortr, btc, btcret = (ctx[i][None, :] for i in range(5))
    with np.errstate(invalid="ignore", divide="ignore"):
        ready = np.isfinite(rsi) & np.isfinite(prsi) & np.isfinite(vma) & np.isfinite(atr) & np.isfinite(ama) \
            & np.isfinite(trend)
        rng = h - l
        wick = (h - np.where(c > o, c, o)) / rng   # max(open_, close)
        setup = (rsi >= P["rsi_short_min"]) & (rsi < prsi) & (c >= bb_upper) & (c < o) & (wick >= P["min_wick_ratio"])
        checks = (   # the last one that holds wins: listed in reverse order of the method
            (SYMBOL_TREND_UP, sym["ok"] & (sym["micro_regime"] == TREND_UP) & (sym["trend_score"] > 0)),
            (BREAKOUT_UP, sym["ok"] & (sym["micro_transition"] == BREAKOUT_UP_CODE)),
            (BTC_UP, np.broadcast_to((btc > 0.15) & (btcret > 0), (S, T))),
            (LONG_EDGE, np.broadcast_to(longr > shortr + P["max_gap"], (S, T))),
            (SYMBOL_ATR, sym["ok"] & (sym["atr_pct"] > P["max_symbol_atr_pct"])),
            (STRESS, np.broadcast_to(stress >= P["max_market_stress"], (S, T))),
            (NO_CONTEXT, np.broadcast_to(~ok[None, :], (S, T))),
            (TREND_TOO_HIGH, trend > P["max_trend_score"]),
            (NO_SETUP, ~setup),
            (BAD_RANGE, rng <= 0),
            (LOW_VOLUME, v < P["volume_ratio_min"] * vma),
            (ATR_SPIKE, atr >= P["atr_spike_max"] * ama),
            (NOT_READY, ~ready))
    status = np.full((S, T), EMIT, np.uint8)
    for code, m in checks:
        status[m] = code
    return status


def replay(o, h, l, c, v, atr, bb_upper, open_time, ctx, ctx_ok=None, *, sym=None, features_given=None, state=None,
           first_t=None, lens=None, from_t=None, **params):
    """Column t of row s = signal() on the message whose frame is
    df.iloc[first_t[s]:t + 1], after the messages of all earlier candles.
    sym: None or {SYM_KEYS: [S] or [S, T]}; features_given: None or
    {FEATURES: [S, T]}; state: None or (has bool [S], last int64 [S]); returns
    the state after."""
    P = {**DEFAULTS, **params}
    S, T = c.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    frm = np.zeros(S, np.int64) if from_t is None else np.clip(np.asarray(from_t, np.int64), 0, T)
    frm = np.maximum(frm, first)
    ft = features_given if features_given is not None else features(c, v, atr, first, ln, P)
    ctx = np.broadcast_to(ctx, (5, T))
    ok = np.ones(T, bool) if ctx_ok is None else np.broadcast_to(np.asarray(ctx_ok).astype(bool), (T,))
    if sym is None:
        sy = dict(ok=np.zeros((S, T), bool), atr_pct=np.zeros((S, T)), trend_score=np.zeros((S, T)),
                  micro_regime=np.full((S, T), NONE), micro_transition=np.full((S, T), NONE))
    else:
        sy = {k: np.broadcast_to(np.asarray(sym[k])[:, None] if np.asarray(sym[k]).ndim == 1 else np.asarray(sym[k]),
                                 (S, T)) for k in SYM_KEYS}
        sy["ok"] = sy["ok"].astype(bool)
    t = np.arange(T)[None, :]
    valid = (t >= frm[:, None]) & (t < ln[:, None])
    status = gates(o, h, l, c, v, atr, bb_upper, ft, ctx, ok, sy, P)
    status[~valid] = NO_FRAME
    sl = stop_loss_pct(atr, c, P)
    has = np.zeros(S, bool) if state is None else np.array(state[0]).astype(bool)
    last = np.zeros(S, np.int64) if state is None else np.array(state[1], np.int64)
    for s, u in zip(*np.nonzero(status == EMIT)):   # row-major: ascending t within a row
        if has[s] and last[s] == open_time[s, u]:            # :291
            status[s, u] = ALREADY_EMITTED
        elif sl[s, u] > P["max_entry_stop_loss_pct"]:        # :297
            status[s, u] = STOP_TOO_WIDE
        else:                                                # :300
            has[s], last[s] = True, open_time[s, u]
    out = {k: np.where(valid, ft[k], np.nan) for k in FEATURES}
    out["stop_loss_pct"] = np.where((status == EMIT) | (status == STOP_TOO_WIDE), sl, np.nan)
    out["score"] = np.where(status == EMIT, score(ft["rsi"], P), np.nan)
    out.update(status=status, state=(has, np.where(has, last, 0)))
    return out
