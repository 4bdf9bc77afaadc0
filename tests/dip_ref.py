"""numpy / pandas restatement of BuyTheDip's decisions, pinned to the recorded
fixture (tests/golden/dip_gates.npz) by test_dip_ref.py and used as the
oracle of the GPU tests.

replay    BuyTheDip.signal() (strategies/coinrule/buy_the_dip.py:127-181)
          message by message over an [S, T] panel; the reference candle is
          found as the method finds it, by scanning the frame backwards
routing   _allows_buy_the_dip_autotrade and _resolve_autotrade_route (:87-125)

Point-wise arithmetic is numpy float64 in the method's operation order, which
is the Python floats' arithmetic bit for bit.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

DEFAULTS = dict(lookback_candles=24, lookback_ms=6 * 3_600_000, start_time_ms=1_776_036_060_000,
                min_change_pct=-5.0, max_change_pct=-2.0, ema_span=20)
(EMIT, NO_FRAME, NOT_READY, BEFORE_START, NO_REFERENCE, OUT_OF_BAND, REGIME_BLOCKED, NOT_RECLAIMED) = range(8)
REASONS = ("emit", "no_frame", "not_enough_data", "before_start_time", "no_reference_price",
           "change_outside_dip_band", "blocked_trend_regime", "prior_close_and_ema20_not_reclaimed")
VALUES = ("reference_price", "change_6h", "ema20")

MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high")
                 + tuple(f"market_regime_{r.lower()}" for r in MARKET_REGIMES) + ("market_regime_none",)
                 + ("symbol_regime_unavailable",) + tuple(f"symbol_regime_{r.lower()}" for r in MICRO_REGIMES))
TRENDS = ("TREND_DOWN", "TREND_UP")


def ema20s(close, first_t=None, lens=None, span=DEFAULTS["ema_span"]):
    """The method's ema20 (:65-70) for every prefix frame: ewm is causal, so
    one ewm over df.iloc[first:] holds every frame's last value."""
    S, T = close.shape
    out = np.full((S, T), np.nan)
    for s in range(S):
        f = 0 if first_t is None else int(first_t[s])
        n = T if lens is None else int(lens[s])
        if f < n:
            out[s, f:n] = pd.Series(close[s, f:n]).ewm(span=span, adjust=False, min_periods=1).mean().to_numpy()
    return out


def find_reference(close_time, first, t, target):
    """_find_reference_price (:49-57): the frame df.iloc[first:t + 1] scanned from its newest row."""
    for u in range(t, first - 1, -1):
        if close_time[u] <= target:
            return u
    return -1


def replay(close, close_time, market_regime=None, micro_regime=None, *, ema20=None, first_t=None, lens=None,
           from_t=None, **params):
    """Column t of row s = signal() on the message whose frame is
    df.iloc[first_t[s]:t + 1]. market_regime: None or int codes [1] / [T];
    micro_regime: None or int codes [S] / [S, T] (negative: None). Returns
    status, the VALUES (NaN where the method did not reach them) and
    reference_index (the reference candle, -1 where there is none)."""
    P = {**DEFAULTS, **params}
    S, T = close.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    frm = np.zeros(S, np.int64) if from_t is None else np.clip(np.asarray(from_t, np.int64), 0, T)
    frm = np.maximum(frm, first)
    if ema20 is None:
        ema20 = ema20s(close, first, ln, P["ema_span"])
    mkt = np.full(T, -1) if market_regime is None else np.broadcast_to(np.asarray(market_regime).reshape(-1), (T,))
    mic = np.full((S, T), -1) if micro_regime is None else np.broadcast_to(
        np.asarray(micro_regime).reshape(S, -1), (S, T))
    trend = [i for i, r in enumerate(MARKET_REGIMES) if r in TRENDS], [i for i, r in enumerate(MICRO_REGIMES)
                                                                       if r in TRENDS]
    status = np.full((S, T), NO_FRAME, np.uint8)
    out = {k: np.full((S, T), np.nan) for k in VALUES}
    ref_index = np.full((S, T), -1, np.int64)
    for s in range(S):
        f = int(first[s])
        null = np.isnan(close[s])
        null[:f] = False
        seen = np.cumsum(null) > 0   # :139 a NaN anywhere in the frame
        ct = close_time[s].tolist()
        for t in range(int(frm[s]), int(ln[s])):
            c = close[s, t]
            if t + 1 - f < P["lookback_candles"] or seen[t]:
                status[s, t] = NOT_READY
                continue
            now = ct[t]
            if now < P["start_time_ms"]:
                status[s, t] = BEFORE_START
                continue
            u = find_reference(ct, f, t, now - P["lookback_ms"])
            if u < 0:
                status[s, t] = NO_REFERENCE
                continue
            ref = close[s, u]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                change = 0.0 if ref == 0 else (c - ref) / abs(ref)   # safe_pct
                change = change * 100.0
            ref_index[s, t] = u
            out["reference_price"][s, t], out["change_6h"][s, t] = ref, change
            if change > P["max_change_pct"] or change <= P["min_change_pct"]:   # a NaN goes on
                status[s, t] = OUT_OF_BAND
            elif mkt[t] in trend[0] or mic[s, t] in trend[1]:
                status[s, t] = REGIME_BLOCKED
            else:
                out["ema20"][s, t] = ema20[s, t]
                reclaimed = c > close[s, t - 1] and c > ema20[s, t]
                status[s, t] = EMIT if reclaimed else NOT_RECLAIMED
    out.update(status=status, reference_index=ref_index)
    return out


def routing(context_ok, transitioning, stress, market_regime, features_ok, micro_regime, max_stress=0.35):
    """(autotrade bool, route code) per element (codes: negative = None);
    arrays broadcast against each other."""
    R = ROUTE_REASONS.index
    args = np.broadcast_arrays(context_ok, transitioning, stress, market_regime, features_ok, micro_regime)
    auto = np.zeros(args[0].shape, bool)
    code = np.zeros(args[0].shape, np.uint8)
    for i in np.ndindex(auto.shape):
        cok, tr, st, mk, fok, mr = (a[i] for a in args)
        market = MARKET_REGIMES[mk] if mk >= 0 else None
        micro = MICRO_REGIMES[mr] if mr >= 0 else None
        if not cok:
            auto[i], code[i] = False, R("market_context_unavailable")
        elif tr:
            auto[i], code[i] = False, R("market_transitioning")
        elif st >= max_stress:
            auto[i], code[i] = False, R("market_stress_too_high")
        elif market not in ("RANGE", "TRANSITIONAL"):
            auto[i], code[i] = False, R(f"market_regime_{str(market).lower()}")
        elif not fok:
            auto[i], code[i] = True, R("symbol_regime_unavailable")
        elif micro is None:
            auto[i], code[i] = False, R("symbol_regime_unavailable")
        else:
            auto[i], code[i] = micro in ("RANGE", "TRANSITIONAL"), R(f"symbol_regime_{micro.lower()}")
    return auto, code
