"""Plain serial numpy restatement of GradualGainerRetest.signal()'s watchlist
state machine (strategies/gradual_gainer_retest.py:222-308), pinned to the
REAL method by tests/golden/retest_gates.npz (tests/test_retest_ref.py) and
used as the oracle of the device kernel (bq_retest_replay) at shapes the
fixture does not hold.

One candle at a time, one row at a time, Python floats: every test is the
method's own expression (one multiply, one compare, in its direction)."""

from __future__ import annotations

import numpy as np

(RT_IDLE, RT_WATCH_SET, RT_WATCHING, RT_RISK_BLOCKED, RT_CANDIDATE, RT_SHORT_HISTORY) = range(6)
RT_NO_FRAME = 255
RT_EVENTS = ("idle", "watch_set", "watching", "risk_blocked", "candidate", "history_too_short")
D_SUPPORT, D_PULLBACK, D_RECLAIM, D_EXPIRED = 1, 2, 4, 8

DEFAULTS = dict(watch_ms=8 * 3_600_000, min_history=100, breakout_lookback=8,
                support_factor=1 - 0.5 / 100, pullback_factor=1 - 0.04)


def nanmax_or_nan(x: np.ndarray) -> float:
    """pandas' Series.max(): NaN skipped, NaN only if all are NaN."""
    x = x[~np.isnan(x)]
    return float(x.max()) if len(x) else float("nan")


def retest_replay(o, h, l, c, ema, open_time, leader, risk_ok=None, *, first_t=None, lens=None, from_t=None,
                  state=None, trace=False, **params):
    """Returns (event uint8 [S, T], detail uint8 [S, T], level [S, T], state)
    with state = (active bool [S], started int64 [S], level [S]) after each
    row's last replayed candle (started 0 / level NaN where idle). `state`:
    the carried-in triple (not modified; None: idle). trace=True adds a
    fifth value: the state after EVERY candle, (active [S, T], started
    [S, T], level [S, T]) — candles not replayed repeat the state before
    them."""
    bad = set(params) - set(DEFAULTS)
    assert not bad, bad
    P = {**DEFAULTS, **params}
    L, mh, watch, sf, pf = (int(P["breakout_lookback"]), int(P["min_history"]), int(P["watch_ms"]),
                            float(P["support_factor"]), float(P["pullback_factor"]))
    assert 1 <= L <= 64 and L < mh
    S, T = c.shape
    ev = np.full((S, T), RT_NO_FRAME, np.uint8)
    dt = np.zeros((S, T), np.uint8)
    lv = np.full((S, T), np.nan)
    act = np.zeros(S, bool) if state is None else np.array(state[0], bool)
    sta = np.zeros(S, np.int64) if state is None else np.array(state[1], np.int64)
    lev = np.full(S, np.nan) if state is None else np.array(state[2], np.float64)
    tr = (np.zeros((S, T), bool), np.zeros((S, T), np.int64), np.full((S, T), np.nan))
    for s in range(S):
        first = 0 if first_t is None else min(max(int(first_t[s]), 0), T)
        n = T if lens is None else min(max(int(lens[s]), 0), T)
        f = 0 if from_t is None else min(max(int(from_t[s]), 0), T)
        active, started, level = bool(act[s]), int(sta[s]), float(lev[s])
        for t in range(T):
            if f <= t < n:
                if t + 1 - first < mh:
                    ev[s, t] = RT_SHORT_HISTORY
                else:
                    ot = int(open_time[s, t])
                    if active and ot > started + watch:
                        active, started, level = False, 0, float("nan")
                        dt[s, t] |= D_EXPIRED
                    if not active and leader[s, t]:
                        active, started, level = True, ot, nanmax_or_nan(np.asarray(h[s, t - L:t], np.float64))
                        ev[s, t], lv[s, t] = RT_WATCH_SET, level
                    elif not active:
                        ev[s, t] = RT_IDLE
                    else:
                        low1, close1, high1, ema1 = float(l[s, t - 1]), float(c[s, t - 1]), float(h[s, t - 1]), \
                            float(ema[s, t - 1])
                        support = low1 >= level * sf or low1 >= ema1 * sf
                        pullback = close1 >= level * pf
                        reclaim = float(c[s, t]) > float(o[s, t]) and float(c[s, t]) > high1
                        lv[s, t] = level
                        if not support or not pullback or not reclaim:
                            ev[s, t] = RT_WATCHING
                            dt[s, t] = (0 if support else D_SUPPORT) | (0 if pullback else D_PULLBACK) \
                                | (0 if reclaim else D_RECLAIM)
                        elif risk_ok is not None and not risk_ok[s, t]:
                            ev[s, t] = RT_RISK_BLOCKED
                        else:
                            ev[s, t] = RT_CANDIDATE
                            active, started, level = False, 0, float("nan")
            tr[0][s, t], tr[1][s, t], tr[2][s, t] = active, started, level
        act[s], sta[s], lev[s] = active, started, level
    out = (ev, dt, lv, (act, sta, lev))
    return out + (tr,) if trace else out


# GradualGainerRetest._risk_allows' reasons (:198-215), the first failing check in the method's order
RISK_REASONS = ("risk_profile_allows_long", "market_context_unavailable", "market_stress_too_high", "btc_context_down",
                "symbol_regime_unavailable", "symbol_atr_too_high", "symbol_transition_not_long", "symbol_trend_down")
