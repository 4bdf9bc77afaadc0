"""numpy restatement of LiquidationSweepPump's candidate gate, rank score,
routing and the portfolio selector's pick (strategies/liquidation_sweep_pump.py
:271-343, :164-193, :78-81), pinned to the real methods by
tests/test_sweep_ref.py on tests/golden/sweep_gates.npz and used as the
reference of the device kernel (tests/test_sweep_gpu.py).

Column u of a [S, T] panel is the TRIGGER candle: the decision signal() takes
on df.iloc[-2] at the message whose frame is df.iloc[first : u + 2]."""

from __future__ import annotations

import numpy as np

COLUMNS = ("pump_score", "score_threshold", "momentum_atr", "close", "prior_high", "close_location",
           "relative_volume", "volume_threshold", "trend_score", "ema20", "relative_strength", "btc_momentum_3",
           "btc_trend_score")   # _is_candidate's required_values, in its order (:272-286)
REASONS = ("candidate", "frame_too_short", "required_value_not_finite", "no_score_cross",
           "momentum_atr_out_of_range", "close_not_above_prior_high", "close_location_too_low",
           "relative_volume_below_threshold", "trend_score_not_positive", "close_not_above_ema20",
           "relative_strength_not_positive", "btc_momentum_not_positive", "btc_trend_not_positive",
           "score_threshold_not_positive", "route_refused")
(CANDIDATE, SHORT_FRAME, NOT_FINITE, NO_CROSS, MOMENTUM_ATR, NOT_ABOVE_PRIOR_HIGH, CLOSE_LOCATION, VOLUME, TREND,
 BELOW_EMA20, RELATIVE_STRENGTH, BTC_MOMENTUM, BTC_TREND, THRESHOLD_NONPOSITIVE, ROUTE_REFUSED) = range(15)
NO_FRAME = 255
DEFAULTS = dict(min_momentum_atr=0.75, max_momentum_atr=3.0, min_close_location=0.70, min_frame=48 + 6 + 2)
ROUTE_REASONS = ("market_context_unavailable", "market_stress_too_high", "market_breadth_not_washed_out",
                 "market_breadth_not_recovering", "btc_not_increasing", "symbol_regime_unavailable",
                 "symbol_trend_not_up", "market_breadth_recovering_btc_up_symbol_up")
ROUTE_OK = len(ROUTE_REASONS) - 1


def gate(cols, score_cross, route_ok=None, first_t=None, lens=None, **thresholds):
    """(status uint8 [S, T], rank_score [S, T]): the first failing check in
    signal()'s order, and pump_score / score_threshold where status == 0 (NaN
    elsewhere). cols: mapping of COLUMNS to [S, T] float64."""
    par = {**DEFAULTS, **thresholds}
    x = [np.asarray(cols[k], np.float64) for k in COLUMNS]
    ps, thr, matr, close, ph, cl, rv, vthr, trend, ema20, rs, bm, bt = x
    S, T = ps.shape
    u = np.arange(T)[None, :]
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t, np.int64)
    ln = np.full(S, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    first, ln = first[:, None], ln[:, None]
    fin = np.ones((S, T), bool)
    for v in x:
        fin &= np.isfinite(v)
    route = np.ones((S, T), bool) if route_ok is None else np.asarray(route_ok, bool)
    with np.errstate(all="ignore"):
        checks = [   # (passes, the code where it does not), the method's order
            (u + 2 - first >= par["min_frame"], SHORT_FRAME),                                 # :314
            (fin, NOT_FINITE),                                                                # :287
            (np.asarray(score_cross, bool), NO_CROSS),                                        # :290
            ((par["min_momentum_atr"] <= matr) & (matr <= par["max_momentum_atr"]), MOMENTUM_ATR),
            (close > ph, NOT_ABOVE_PRIOR_HIGH), (cl >= par["min_close_location"], CLOSE_LOCATION),
            (rv >= vthr, VOLUME), (trend > 0, TREND), (close > ema20, BELOW_EMA20), (rs > 0, RELATIVE_STRENGTH),
            (bm > 0, BTC_MOMENTUM), (bt > 0, BTC_TREND),                                       # :291-299
            (~(thr <= 0), THRESHOLD_NONPOSITIVE),                                              # :331
            (route, ROUTE_REFUSED),                                                           # :343
        ]
        status = np.zeros((S, T), np.uint8)
        for ok, code in reversed(checks):
            status = np.where(ok, status, np.uint8(code))
        status = np.where((u + 1 >= ln) | (u < first), np.uint8(NO_FRAME), status).astype(np.uint8)
        rank = np.where(status == 0, ps / thr, np.nan)
    return status, rank


def winners(status, rank_score, symbol_rank=None):
    """(winner int64 [T], winner_score [T]): per column the candidate with the
    largest (rank_score, symbol_rank, row) — _dispatch_winner's
    max(key=(rank_score, symbol)) (:78-81); -1 / NaN without a candidate."""
    S, T = status.shape
    sr = np.arange(S) if symbol_rank is None else np.asarray(symbol_rank)
    win, score = np.full(T, -1, np.int64), np.full(T, np.nan)
    for t in range(T):
        rows = np.flatnonzero(status[:, t] == 0)
        if len(rows):
            w = max(rows, key=lambda s: (rank_score[s, t], sr[s], s))
            win[t], score[t] = w, rank_score[w, t]
    return win, score


def select(cols, score_cross, route_ok=None, first_t=None, lens=None, symbol_rank=None, **thresholds):
    status, rank = gate(cols, score_cross, route_ok, first_t, lens, **thresholds)
    win, score = winners(status, rank, symbol_rank)
    return {"status": status, "candidate": status == 0, "rank_score": rank, "winner": win, "winner_score": score}


def symbol_ranks(names) -> np.ndarray:
    """int32 [S]: each name's position in Python's str order of the names."""
    names = [str(n) for n in names]
    order = sorted(range(len(names)), key=lambda i: names[i])
    rank = np.zeros(len(names), np.int32)
    rank[order] = np.arange(len(names), dtype=np.int32)
    return rank


def routing(stress, breadth, recovery, context_ok, btc_momentum, trend, features_ok, max_market_stress=0.35,
            breadth_threshold=-0.2, min_breadth_recovery=0.02):
    """long_entry_routing (:164-193) element-wise: the reason's index in
    ROUTE_REASONS (uint8). recovery NaN = the method's None."""
    stress, breadth, recovery, btc_momentum, trend = (np.asarray(v, np.float64) for v in (
        stress, breadth, recovery, btc_momentum, trend))
    with np.errstate(all="ignore"):
        checks = [(~np.asarray(context_ok, bool), 0), (stress >= max_market_stress, 1),
                  (breadth > breadth_threshold, 2), (np.isnan(recovery) | (recovery < min_breadth_recovery), 3),
                  (btc_momentum <= 0, 4), (~np.asarray(features_ok, bool), 5), (trend <= 0, 6)]
    code = np.full(np.broadcast(*[c for c, _ in checks]).shape, ROUTE_OK, np.uint8)
    for cond, value in reversed(checks):
        code = np.where(cond, np.uint8(value), code)
    return code.astype(np.uint8)
