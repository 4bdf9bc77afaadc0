"""numpy restatement of BBExtremeReversion's decisions, pinned to the recorded
fixture (tests/golden/bbextreme_gates.npz) by test_bbextreme_ref.py and used as
the oracle of the GPU tests.

roll_mean_last  pandas' rolling(window).mean() (2.3.3, roll_mean in
                _libs/window/aggregations.pyx, fixed windows, min_periods =
                window) at the last row of a frame: the online add / remove
                sum with its two Kahan compensations, started at the frame's
                first row
frame_rsi       _compute_rsi (strategies/coinrule/bb_extreme_reversion.py
                :134-150) on one frame's closes
replay          signal() with ENABLED true (:234-285, evaluate :152-232)
                message by message over an [S, T] panel
routing         supports_autotrade and _resolve_directional_autotrade (:86-132)

Every operation is the IEEE float64 operation the method performs, in its
order: the values equal the recording bit for bit.
"""

from __future__ import annotations

import math

import numpy as np

DEFAULTS = dict(lookback=30, rsi_window=2, oversold_rsi=5.0, overbought_rsi=95.0, max_lower_band_position=0.0,
                min_upper_band_position=1.0)
(EMIT, NO_FRAME, NOT_ENOUGH_DATA, NULLS, NO_RSI, INVALID_BAND, NO_EXTREME) = range(7)
REASONS = ("emit", "no_frame", "not_enough_data", "recent_data_contains_nulls", "not_enough_candles_for_rsi",
           "invalid_band_spread", "no_extreme")
VALUES = ("rsi_value", "band_position", "bb_width", "distance_from_mid_pct", "direction")
BUY, SELL = 0.0, 1.0   # bq_direction: LONG, SHORT

MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
BLOCKING_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKDOWN", "ENTERED_TRANSITIONAL")
SHORTABLE = ("RANGE", "TRANSITIONAL", "TREND_DOWN")
ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high")
                 + tuple(f"market_regime_{r.lower()}" for r in MARKET_REGIMES) + ("market_regime_none",)
                 + ("market_range_unstable_allowed", "market_range_stable", "symbol_features_unavailable")
                 + tuple(f"symbol_transition_{r.lower()}" for r in BLOCKING_TRANSITIONS)
                 + ("symbol_micro_regime_unstable", "symbol_regime_not_shortable",
                    "symbol_regime_trend_down_for_long"))

# which of calc_mean's branches formed a mean (roll_mean_last's second result)
PLAIN, SAME_VALUE, NO_NEGATIVE, ALL_NEGATIVE, TOO_FEW = range(5)


def roll_mean_last(values, window: int):
    """(pd.Series(values).rolling(window).mean().iloc[-1], the branch of
    calc_mean that formed it). values: a sequence of floats without NaN."""
    s = ca = cr = 0.0
    nobs = neg = same = 0
    x = [float("nan") if math.isinf(v) else float(v) for v in values]   # _prep_values
    prev = x[0]
    for j, v in enumerate(x):
        if j >= window:   # the window's start moved: remove_mean
            r = x[j - window]
            if r == r:
                nobs -= 1
                y = -r - cr
                t = s + y
                cr = t - s - y
                s = t
                if math.copysign(1.0, r) < 0:
                    neg -= 1
        if v == v:        # add_mean
            nobs += 1
            y = v - ca
            t = s + y
            ca = t - s - y
            s = t
            if math.copysign(1.0, v) < 0:
                neg += 1
            same = same + 1 if v == prev else 1
            prev = v
    if not (nobs >= window and nobs > 0):
        return float("nan"), TOO_FEW
    result = s / nobs
    if same >= nobs:
        return prev, SAME_VALUE
    if neg == 0 and result < 0:
        return 0.0, NO_NEGATIVE
    if neg == nobs and result > 0:
        return 0.0, ALL_NEGATIVE
    return result, PLAIN


def direct_mean_last(values, window: int):
    """The shortcut a frame-local replay must not be: the last window summed
    on its own (inf still missing)."""
    w = [float(v) for v in values[-window:]]
    if len(values) < window or any(math.isinf(v) for v in w):
        return float("nan")
    s = 0.0
    for v in w:
        s = s + v
    return s / window


def gains_losses(closes):
    """delta.where(delta > 0, 0.0) and -delta.where(delta < 0, 0.0) of closes.diff()."""
    c = np.asarray(closes, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.concatenate([[np.nan], c[1:] - c[:-1]])
        gain = np.where(d > 0, d, 0.0)
        loss = -np.where(d < 0, d, 0.0)
    return gain.tolist(), loss.tolist()


def _rsi_of(g: float, q: float):
    with np.errstate(all="ignore"):
        rs = np.float64(g) / np.float64(q)
        val = float(100 - (100 / (1 + rs)))
    if val != val:
        return None
    return max(0.0, min(100.0, val))


def frame_rsi(closes, window: int, hits: list | None = None):
    """_compute_rsi: None, or the clamped RSI. hits: receives the two calc_mean branches."""
    if len(closes) < window + 1:
        return None
    gain, loss = gains_losses(closes)
    g, hg = roll_mean_last(gain, window)
    q, hq = roll_mean_last(loss, window)
    if hits is not None:
        hits[:] = [hg, hq]
    return _rsi_of(g, q)


def frame_rsi_direct(closes, window: int, hits: list | None = None):
    """_compute_rsi with direct window sums in place of roll_mean."""
    if len(closes) < window + 1:
        return None
    gain, loss = gains_losses(closes)
    return _rsi_of(direct_mean_last(gain, window), direct_mean_last(loss, window))


def evaluate(rsi, price: float, hi: float, mid: float, lo: float, P: dict):
    """evaluate (:152-232) given _compute_rsi's result: (status, the VALUES in order)."""
    price, hi, mid, lo = float(price), float(hi), float(mid), float(lo)
    with np.errstate(all="ignore"):
        span = np.float64(hi) - np.float64(lo)
        pos = float((np.float64(price) - np.float64(lo)) / span) if span > 0 else 0.5
        width = float(span / np.float64(mid)) if mid > 0 else 0.0
        dist = float((np.float64(price) - np.float64(mid)) / np.float64(mid) * 100) if mid > 0 else 0.0
    vals = [rsi if rsi is not None else 50.0, pos, width, dist, float("nan")]
    if rsi is None:
        return NO_RSI, vals
    if span <= 0:
        return INVALID_BAND, vals
    if rsi <= P["oversold_rsi"] and pos <= P["max_lower_band_position"]:
        vals[4] = BUY
        return EMIT, vals
    if rsi >= P["overbought_rsi"] and pos >= P["min_upper_band_position"]:
        vals[4] = SELL
        return EMIT, vals
    return NO_EXTREME, vals


def replay(close, bb_upper, bb_mid, bb_lower, *, first_t=None, lens=None, from_t=None, rsi=frame_rsi, **params):
    """Column t of row s = signal() on the message whose frame is
    df.iloc[first_t[s]:t + 1] with current_price = close[t] and the bands of
    candle t. Returns status, the VALUES (NaN where the method did not reach
    evaluate) and mean_rule [S, T, 2] (the calc_mean branch of the gain and
    the loss mean, -1 where _compute_rsi formed none)."""
    P = {**DEFAULTS, **params}
    L, W = int(P["lookback"]), int(P["rsi_window"])
    S, T = close.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    frm = np.zeros(S, np.int64) if from_t is None else np.clip(np.asarray(from_t, np.int64), 0, T)
    frm = np.maximum(frm, first)
    status = np.full((S, T), NO_FRAME, np.uint8)
    out = {k: np.full((S, T), np.nan) for k in VALUES}
    rule = np.full((S, T, 2), -1, np.int8)
    for s in range(S):
        f = int(first[s])
        null = np.isnan(close[s])
        for t in range(int(frm[s]), int(ln[s])):
            if t + 1 - f < L:                       # :255
                status[s, t] = NOT_ENOUGH_DATA
                continue
            if null[t - L + 1:t + 1].any():         # :264
                status[s, t] = NULLS
                continue
            hits = []
            r = rsi(close[s, t - L + 1:t + 1], W, hits)
            if hits:
                rule[s, t] = hits
            status[s, t], vals = evaluate(r, close[s, t], bb_upper[s, t], bb_mid[s, t], bb_lower[s, t], P)
            for k, v in zip(VALUES, vals):
                out[k][s, t] = v
    out.update(status=status, mean_rule=rule)
    return out


def routing(context_ok, transitioning, timestamp, stable_since, stress, market_regime, features_ok, micro_regime,
            micro_transition, strength, direction, stress_threshold=0.35, min_age_ms=30 * 60 * 1000, min_strength=0.5):
    """(autotrade bool, route code) per element (codes: negative = None;
    stable_since negative: None; direction BUY / SELL); arrays broadcast
    against each other."""
    R = ROUTE_REASONS.index
    args = np.broadcast_arrays(context_ok, transitioning, timestamp, stable_since, stress, market_regime, features_ok,
                               micro_regime, micro_transition, strength, direction)
    auto = np.zeros(args[0].shape, bool)
    code = np.zeros(args[0].shape, np.uint8)
    for i in np.ndindex(auto.shape):
        cok, tr, ts, since, st, mk, fok, mr, mt, sg, dr = (a[i] for a in args)
        market = MARKET_REGIMES[mk] if mk >= 0 else None
        micro = MICRO_REGIMES[mr] if mr >= 0 else None
        trans = MICRO_TRANSITIONS[mt] if mt >= 0 else None
        # supports_autotrade
        if not cok:
            ok, route = False, "market_context_unavailable"
        elif tr:
            ok, route = False, "market_transitioning"
        elif st >= stress_threshold:
            ok, route = False, "market_stress_too_high"
        elif market != "RANGE":
            ok, route = False, f"market_regime_{str(market).lower()}"
        elif since < 0 or max(int(ts) - int(since), 0) < min_age_ms:   # is_regime_stable
            ok, route = True, "market_range_unstable_allowed"
        else:
            ok, route = True, "market_range_stable"
        # _resolve_directional_autotrade
        if ok:
            if not fok:
                ok, route = False, "symbol_features_unavailable"
            elif trans in BLOCKING_TRANSITIONS:
                ok, route = False, f"symbol_transition_{trans.lower()}"
            elif sg < min_strength:
                ok, route = False, "symbol_micro_regime_unstable"
            elif dr == SELL and micro not in SHORTABLE:
                ok, route = False, "symbol_regime_not_shortable"
            elif dr == BUY and micro == "TREND_DOWN":
                ok, route = False, "symbol_regime_trend_down_for_long"
        auto[i], code[i] = ok, R(route)
    return auto, code
