"""numpy / pandas restatement of the 5m strategies' decisions, pinned to the
recorded fixture (tests/golden/pricetracker_gates.npz) by
test_pricetracker_ref.py and used as the oracle of the GPU tests.

replay            PriceTracker.signal() (strategies/coinrule/price_tracker.py
                  :165-251) message by message over an [S, T] panel
routing           PriceTracker.regime_routing (:113-163)
long_autotrade    allows_long_autotrade (market_regime/regime_routing.py:47-75)
burst_entry       ActivityBurstPump.signal() (:164-185)

Point-wise arithmetic is numpy float64 in the method's operation order, which
is the Python floats' arithmetic bit for bit.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

DEFAULTS = dict(min_history=30, tail_rows=5, span_fast=9, span_slow=21, rsi_max=30.0, macd_max=0.0, mfi_max=20.0,
                w_rsi=0.35, w_mfi=0.35, w_macd=0.3, macd_scale=100.0, context_weight=0.35, risk_weight=0.35,
                support_weight=0.2, min_followthrough=-0.2, max_risk=0.6, min_confidence=0.5,
                cooldown_ms=12 * 300_000)
(EMIT, NO_FRAME, NOT_READY, NO_SETUP, NO_CONTEXT, CONTEXT_REJECTED, COOLDOWN) = range(7)
D_FOLLOWTHROUGH, D_RISK, D_CONFIDENCE = 1, 2, 4
VALUES = ("local_score", "trend_score", "followthrough", "adverse_risk", "supportiveness", "adjusted_score")
CTX_ROWS = ("confidence", "long_tailwind", "btc_regime_score", "market_stress_score")

MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
ROUTE_REASONS = (("market_context_unavailable", "market_transitioning", "market_stress_too_high",
                  "breadth_not_stable_for_mean_reversion", "market_regime_unavailable")
                 + tuple(f"market_regime_{r.lower()}" for r in MARKET_REGIMES)
                 + ("symbol_regime_unavailable", "symbol_transition_breakdown",
                    "symbol_transition_volatility_expansion", "symbol_relative_strength_vs_btc_insufficient",
                    "symbol_trend_score_outside_range", "symbol_range")
                 + tuple(f"symbol_regime_{r.lower()}" for r in MICRO_REGIMES))
ROUTE_OK = ROUTE_REASONS.index("symbol_range")
(AB_EMIT, AB_NO_FRAME, AB_SHORT_FRAME, AB_ROUTE_REFUSED, AB_NOT_QUALIFIED) = range(5)


def _clamp(x, lo=-1.0, hi=1.0):   # shared/utils.py:12-13: max(low, min(high, value))
    m = np.where(x < hi, x, hi)
    return np.where(m > lo, m, lo)


def _nneg(x):   # max(0.0, value)
    return np.where(x > 0.0, x, 0.0)


def local_score(rsi, macd, mfi, P=DEFAULTS):   # :198-203
    with np.errstate(invalid="ignore"):
        return ((1.0 + _nneg((P["rsi_max"] - rsi) / P["rsi_max"]) * P["w_rsi"])
                + _nneg((P["mfi_max"] - mfi) / P["mfi_max"]) * P["w_mfi"]) \
            + np.where(1.0 < np.abs(macd) * P["macd_scale"], 1.0, np.abs(macd) * P["macd_scale"]) * P["w_macd"]


def context_score(rs, trend, conf, tailwind, btc, stress, ok):
    """RuleBasedMarketContextModel.evaluate, LONG (context_scoring.py:22-85):
    (confidence, followthrough, adverse risk, supportiveness) as the
    MarketContextScore holds them; _empty_score where ok is False or
    confidence <= 0."""
    with np.errstate(invalid="ignore"):
        real = ok & ~(conf <= 0.0)
        btc_al = _clamp(btc)
        cross = _clamp(0.6 * rs + 0.4 * trend)
        over = _clamp(0.6 * _nneg(rs) + 0.4 * _nneg(trend), 0.0, 1.0)
        sup = _clamp(0.35 * tailwind + 0.25 * btc_al + 0.25 * cross + 0.15 * (-stress))
        fol = _clamp(0.45 * tailwind + 0.3 * btc_al + 0.25 * cross)
        adv = _clamp(0.55 * stress + 0.25 * _nneg(-sup) + 0.2 * (1.0 - over), 0.0, 1.0)
        boost = (tailwind < 0.0) & (over > 0.0)
        sup = np.where(boost, _clamp(sup + 0.2 * over), sup)
        fol = np.where(boost, _clamp(fol + 0.15 * over), fol)
    z = np.zeros_like(fol)
    return np.where(real, conf, z), np.where(real, fol, z), np.where(real, adv, z), np.where(real, sup, z)


def trend_scores(close, first_t=None, lens=None, P=DEFAULTS):
    """The method's trend_score (:204-210) for every prefix frame: ewm is
    causal, so one ewm over df.iloc[first:] holds every frame's last value."""
    S, T = close.shape
    out = np.full((S, T), np.nan)
    for s in range(S):
        f = 0 if first_t is None else int(first_t[s])
        n = T if lens is None else int(lens[s])
        if f >= n:
            continue
        c = pd.Series(close[s, f:n])
        fast = c.ewm(span=P["span_fast"], adjust=False).mean().to_numpy()
        slow = c.ewm(span=P["span_slow"], adjust=False).mean().to_numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            out[s, f:n] = np.where(slow != 0, (fast - slow) / np.abs(slow), 0.0)
    return out


def replay(close, rsi, macd, mfi, close_time, symbol_rs, ctx, ctx_ok=None, *, high=None, low=None, volume=None,
           trend_score=None, state=None, first_t=None, lens=None, from_t=None, **params):
    """Column t of row s = signal() on the message whose frame is
    df.iloc[first_t[s]:t + 1], after the messages of all earlier candles.
    state: None or (has bool [S], last int64 [S]); returns the state after."""
    P = {**DEFAULTS, **params}
    S, T = close.shape
    first = np.zeros(S, np.int64) if first_t is None else np.clip(np.asarray(first_t, np.int64), 0, T)
    ln = np.full(S, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    frm = np.zeros(S, np.int64) if from_t is None else np.clip(np.asarray(from_t, np.int64), 0, T)
    frm = np.maximum(frm, first)
    if trend_score is None:
        trend_score = trend_scores(close, first, ln, P)
    rs = np.broadcast_to(symbol_rs[:, None] if symbol_rs.ndim == 1 else symbol_rs, (S, T))
    ctx = np.broadcast_to(ctx, (4, T))
    ok = np.ones(T, bool) if ctx_ok is None else np.broadcast_to(np.asarray(ctx_ok).astype(bool), (T,))
    t = np.arange(T)[None, :]
    valid = (t >= frm[:, None]) & (t < ln[:, None])
    null = np.isnan(close) | np.isnan(rsi) | np.isnan(macd)
    for x in (high, low, volume):
        if x is not None:
            null = null | np.isnan(x)
    null = null & (t >= first[:, None])
    tail = np.zeros((S, T), bool)
    for k in range(P["tail_rows"]):
        tail[:, k:] |= null[:, :T - k]
    ready = (t + 1 - first[:, None] >= P["min_history"]) & ~tail
    with np.errstate(invalid="ignore"):
        setup = (rsi < P["rsi_max"]) & (macd < P["macd_max"]) & (mfi < P["mfi_max"])
        local = local_score(rsi, macd, mfi, P)
        conf, fol, adv, sup = context_score(rs, trend_score, ctx[0][None, :], ctx[1][None, :], ctx[2][None, :],
                                            ctx[3][None, :], ok[None, :])
        adj = local + conf * P["context_weight"] * (fol + (P["support_weight"] * sup) - (P["risk_weight"] * adv))
        rej = ((fol < P["min_followthrough"]) * D_FOLLOWTHROUGH | (adv > P["max_risk"]) * D_RISK
               | (conf < P["min_confidence"]) * D_CONFIDENCE)
    status = np.full((S, T), EMIT, np.uint8)
    status[rej != 0] = CONTEXT_REJECTED
    status[:, ~ok] = NO_CONTEXT
    status[~setup] = NO_SETUP
    status[~ready] = NOT_READY
    status[~valid] = NO_FRAME
    detail = np.where(status == CONTEXT_REJECTED, rej, 0).astype(np.uint8)
    has = np.zeros(S, bool) if state is None else np.array(state[0]).astype(bool)
    last = np.zeros(S, np.int64) if state is None else np.array(state[1], np.int64)
    cd = int(P["cooldown_ms"])
    if cd > 0:
        for s, u in zip(*np.nonzero(status == EMIT)):   # row-major: ascending t within a row
            elapsed = int(close_time[s, u]) - int(last[s])
            if has[s] and 0 <= elapsed < cd:   # :83-93
                status[s, u] = COOLDOWN
            else:                              # :95-99
                has[s], last[s] = True, close_time[s, u]
    reached = (status == EMIT) | (status >= NO_CONTEXT)
    cols = dict(zip(VALUES, (local, trend_score, fol, adv, sup, adj)))
    out = {k: np.where(reached, v, np.nan) for k, v in cols.items()}
    out.update(status=status, detail=detail, state=(has, np.where(has, last, 0)))
    return out


def routing(context_ok, transitioning, stress, advancers_ratio, long_tailwind, short_tailwind, market_regime,
            features_ok, micro_regime, micro_transition, rs, trend, stress_threshold=0.3, min_rs=0.005,
            max_abs_trend=0.005):
    """regime_routing's reason per element (codes: negative = None); arrays
    broadcast against each other."""
    R = ROUTE_REASONS.index
    args = np.broadcast_arrays(context_ok, transitioning, stress, advancers_ratio, long_tailwind, short_tailwind,
                               market_regime, features_ok, micro_regime, micro_transition, rs, trend)
    out = np.zeros(args[0].shape, np.uint8)
    for i in np.ndindex(out.shape):
        cok, tr, st, ar, lt, sht, mk, fok, mr, mt, r, tnd = (a[i] for a in args)
        if not cok:
            code = R("market_context_unavailable")
        elif tr:
            code = R("market_transitioning")
        elif st >= stress_threshold:
            code = R("market_stress_too_high")
        elif not (0.48 <= ar <= 0.62 and abs(lt - sht) <= 0.35):
            code = R("breadth_not_stable_for_mean_reversion")
        elif mk < 0:
            code = R("market_regime_unavailable")
        elif MARKET_REGIMES[mk] != "RANGE":
            code = R("market_regime_" + MARKET_REGIMES[mk].lower())
        elif not fok:
            code = R("symbol_regime_unavailable")
        elif mt >= 0 and MICRO_TRANSITIONS[mt] in ("BREAKDOWN", "VOLATILITY_EXPANSION"):
            code = R("symbol_transition_" + MICRO_TRANSITIONS[mt].lower())
        elif r <= min_rs:
            code = R("symbol_relative_strength_vs_btc_insufficient")
        elif abs(tnd) > max_abs_trend:
            code = R("symbol_trend_score_outside_range")
        elif mr < 0:
            code = R("symbol_regime_unavailable")
        elif MICRO_REGIMES[mr] == "RANGE":
            code = ROUTE_OK
        else:
            code = R("symbol_regime_" + MICRO_REGIMES[mr].lower())
        out[i] = code
    return out


def long_autotrade(context_ok, transitioning, timestamp, stable_since, market_regime, stress, features_ok,
                   micro_regime, micro_transition, min_age_ms=30 * 60 * 1000):
    """allows_long_autotrade per element (stable_since negative: None)."""
    args = np.broadcast_arrays(context_ok, transitioning, timestamp, stable_since, market_regime, stress,
                               features_ok, micro_regime, micro_transition)
    out = np.zeros(args[0].shape, bool)
    for i in np.ndindex(out.shape):
        cok, tr, ts, since, mk, st, fok, mr, mt = (a[i] for a in args)
        regime = MARKET_REGIMES[mk] if mk >= 0 else None
        if not cok or tr or since < 0 or max(int(ts) - int(since), 0) < min_age_ms:
            ok = False
        elif regime in ("HIGH_STRESS", "TREND_DOWN", "TRANSITIONAL") or st >= 0.35:
            ok = False
        elif not fok:
            ok = regime in ("TREND_UP", "RANGE")
        elif mr >= 0 and MICRO_REGIMES[mr] == "TREND_DOWN":
            ok = mt >= 0 and MICRO_TRANSITIONS[mt] == "RECOVERY"
        else:
            ok = mr >= 0 and MICRO_REGIMES[mr] in ("TREND_UP", "RANGE", "TRANSITIONAL")
        out[i] = ok
    return out


def burst_entry(qualified, route_ok, ctx_ok, first_t=None, lens=None, min_rows=21):
    """ActivityBurstPump.signal() :164-185: (status, autotrade) per cell."""
    S, T = qualified.shape
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t, np.int64)
    ln = np.full(S, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    t = np.arange(T)[None, :]
    route_ok = np.broadcast_to(route_ok, (S, T))
    ctx_ok = np.broadcast_to(np.asarray(ctx_ok, bool).reshape(1, -1), (S, T))
    status = np.full((S, T), AB_EMIT, np.uint8)
    status[~qualified] = AB_NOT_QUALIFIED
    status[ctx_ok & ~route_ok] = AB_ROUTE_REFUSED
    status[t + 1 - first[:, None] < min_rows] = AB_SHORT_FRAME
    status[(t < first[:, None]) | (t >= ln[:, None])] = AB_NO_FRAME
    return status, (status == AB_EMIT) & ctx_ok
