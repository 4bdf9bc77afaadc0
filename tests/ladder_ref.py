"""numpy restatement of LadderDeployer.signal()
(strategies/grid/ladder_deployer.py:58-187 with _bb_stable :42-56) on the
frames df_15m.iloc[first:t + 1], and of GridOnlyPolicy.resolve after
_breadth_pair (market_regime/grid_only_policy.py:121-158): the oracle of the
GPU tests, pinned to what the real classes did by
tests/golden/ladder_gates.npz (tests/test_ladder_ref.py).

Every value is the method's IEEE operation sequence applied element-wise
(numpy's float64 +, -, *, / are the same correctly rounded operations as
Python's), and Python's min / max are written as the selects they are: the
first argument unless the second compares strictly beyond it.
"""

from __future__ import annotations

import numpy as np

DEFAULTS = dict(n=8, max_change_pct=20.0, min_width_pct=1.5, max_width_pct=8.0, min_buffer_pct=0.5,
                max_buffer_pct=4.0, atr_multiplier=1.5, min_long_score=0.2)
(EMIT, NO_FRAME, POLICY, NO_CONTEXT, NOT_RANGE, MICRO_REGIME, SYMBOL_TRANSITION, BELOW_EMAS, RS_NOT_POSITIVE,
 LONG_SCORE_LOW, BB_EXPANDING, PRICE_OUTSIDE, RANGE_WIDTH) = range(13)
REASONS = ("emit", "no_frame", "grid_only_policy", "market_context_unavailable", "market_regime_not_range",
           "symbol_micro_regime", "symbol_transition", "symbol_below_ema20_and_ema50",
           "relative_strength_vs_btc_not_positive", "long_regime_score_too_low", "bb_width_expanding",
           "price_outside_range", "range_width")
VALUES = ("bb_change_pct", "range_width_pct", "breakout_buffer_pct", "breakout_low", "breakout_high")
SYM_KEYS = ("ok", "micro_regime", "micro_transition", "above_ema20", "above_ema50", "rs_vs_btc", "atr_pct")
MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
BLOCKING_TRANSITIONS = ("BREAKDOWN", "VOLATILITY_EXPANSION", "ENTERED_TREND_DOWN")
RANGE = 2            # "RANGE" in both MARKET_REGIMES and MICRO_REGIMES
NONE = 255           # a None micro_regime / micro_regime_transition
MAX_N = 64
TILE = 1024          # the kernel's tile width (binquant_amd._lib.GRID_LADDER_TILE)

GRID_ONLY_REGIMES = ("RANGE", "TRANSITIONAL")
POLICY_REASONS = (("market_context_unavailable", "market_regime_unavailable")
                  + tuple(f"market_regime_{r.lower()}" for r in MARKET_REGIMES if r not in GRID_ONLY_REGIMES)
                  + ("breadth_momentum_unavailable", "breadth_momentum_toward_trend", "breadth_momentum_toward_range",
                     "breadth_momentum_flat"))


def _rows(v, S, default):
    return np.full(S, default, np.int64) if v is None else np.asarray(v, np.int64).reshape(S)


def py_max(a, b):
    return np.where(b > a, b, a)


def py_min(a, b):
    return np.where(b < a, b, a)


def bb_stable(bb_upper, bb_mid, bb_lower, n: int, max_change_pct: float, first):
    """_bb_stable on every frame df.iloc[first[s]:t + 1]: (verdict bool [S, T],
    change_pct [S, T], NaN where the method returns before :55)."""
    up, md, lw = (np.asarray(x, np.float64) for x in (bb_upper, bb_mid, bb_lower))
    S, T = md.shape
    with np.errstate(all="ignore"):
        w = (up - lw) / md
        bad = (md <= 0) | (w <= 0)                      # :49-53; a NaN row passes both tests
    nbad = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(bad, axis=1)], axis=1)
    t = np.arange(T)
    lo = t - (n - 1)
    enough = (t[None, :] + 1 - np.asarray(first).reshape(S, 1)) >= n        # :44
    lo_c = np.clip(lo, 0, None)
    clean = (nbad[:, t + 1] - nbad[:, lo_c]) == 0
    reached = enough & clean
    with np.errstate(all="ignore"):
        w0 = w[:, lo_c]
        change = np.abs((w - w0) / w0) * 100            # :55
        verdict = reached & (change <= max_change_pct)
    return verdict, np.where(reached, change, np.nan)


def replay(close, bb_upper, bb_mid, bb_lower, market_regime, long_regime_score, ctx_ok=None, policy_ok=None, *,
           bands=None, sym=None, first_t=None, lens=None, from_t=None, **params) -> dict:
    """status uint8 [S, T] and the five value columns [S, T]. The context arrays
    have 1 or T entries; sym is None (no symbol has features) or {SYM_KEYS:
    array}, [S] or [S, T]; bands None: the frame's columns."""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    P = {**DEFAULTS, **params}
    n = int(P["n"])
    assert 1 <= n <= MAX_N
    price = np.asarray(close, np.float64)
    S, T = price.shape
    first, ln, frm = _rows(first_t, S, 0).clip(0, T), _rows(lens, S, T).clip(0, T), _rows(from_t, S, 0).clip(0, T)
    high, mid, low = (np.asarray(x, np.float64) for x in (bands if bands is not None else (bb_upper, bb_mid, bb_lower)))
    ctx = lambda a, dflt: np.broadcast_to(np.asarray(dflt if a is None else a).reshape(-1), (T,))[None, :]   # noqa: E731
    pok, cok = ctx(policy_ok, True).astype(bool), ctx(ctx_ok, True).astype(bool)
    regime, score = ctx(market_regime, 0).astype(np.int64), ctx(long_regime_score, 0.0).astype(np.float64)
    if sym is None:
        sok = np.zeros((S, T), bool)
        sreg = strans = np.full((S, T), NONE)
        e20 = e50 = sok
        rs = atr = np.zeros((S, T))
    else:
        sy = [np.broadcast_to(np.asarray(sym[k]).reshape(S, -1), (S, T)) for k in SYM_KEYS]
        sok, sreg, strans, e20, e50 = sy[0].astype(bool), sy[1], sy[2], sy[3].astype(bool), sy[4].astype(bool)
        rs, atr = sy[5].astype(np.float64), sy[6].astype(np.float64)
    verdict, change = bb_stable(bb_upper, bb_mid, bb_lower, n, float(P["max_change_pct"]), first)
    t = np.arange(T)[None, :]
    with np.errstate(all="ignore"):
        rw = np.where(mid > 0, ((high - low) / mid) * 100, 0.0)                        # :112-114
        raw = atr * 100 * P["atr_multiplier"]                                          # :120
        buf = py_max(P["min_buffer_pct"], py_min(P["max_buffer_pct"], raw))            # :121-124
        blow, bhigh = low * (1 - buf / 100), high * (1 + buf / 100)                    # :150-151
        blocked = np.isin(strans, [MICRO_TRANSITIONS.index(x) for x in BLOCKING_TRANSITIONS])
        checks = [                                                                     # the method's order
            ((t < np.maximum(frm, first)[:, None]) | (t >= ln[:, None]), NO_FRAME),
            (~pok, POLICY),                                                            # :70
            (~cok, NO_CONTEXT),                                                        # :76
            (regime != RANGE, NOT_RANGE),                                              # :79
            (~sok | (sreg != RANGE), MICRO_REGIME),                                    # :83-88
            (blocked, SYMBOL_TRANSITION),                                              # :89
            (~e20 & ~e50, BELOW_EMAS),                                                 # :92
            (rs <= 0, RS_NOT_POSITIVE),                                                # :95
            (score < P["min_long_score"], LONG_SCORE_LOW),                             # :98
            (~verdict, BB_EXPANDING),                                                  # :101
            (~((low < price) & (price < high)), PRICE_OUTSIDE),                        # :109
            (~((P["min_width_pct"] <= rw) & (rw <= P["max_width_pct"])), RANGE_WIDTH),  # :115
        ]
    status = np.full((S, T), EMIT, np.uint8)
    for cond, code in reversed(checks):
        status = np.where(np.broadcast_to(cond, (S, T)), np.uint8(code), status)
    emit = status == EMIT
    walked = emit | (status >= BB_EXPANDING)
    nan = np.nan
    return dict(status=status, bb_change_pct=np.where(walked, change, nan),
                range_width_pct=np.where(emit | (status == RANGE_WIDTH), rw, nan),
                breakout_buffer_pct=np.where(emit, buf, nan), breakout_low=np.where(emit, blow, nan),
                breakout_high=np.where(emit, bhigh, nan))


def grid_only_policy(context_ok, market_regime, previous, latest):
    """(allow bool, reason uint8 (POLICY_REASONS' index), momentum_points)."""
    cok = np.asarray(context_ok).astype(bool)
    mk = np.asarray(market_regime).astype(np.int64)
    prev, lat = np.asarray(previous, np.float64), np.asarray(latest, np.float64)
    R = POLICY_REASONS.index
    family = np.zeros(mk.shape, np.int64)
    for r in MARKET_REGIMES:
        if r not in GRID_ONLY_REGIMES:
            family = np.where(mk == MARKET_REGIMES.index(r), R("market_regime_" + r.lower()), family)
    grid = np.isin(mk, [MARKET_REGIMES.index(r) for r in GRID_ONLY_REGIMES])
    la, pa = np.abs(lat), np.abs(prev)
    checks = [(~cok, R("market_context_unavailable")), (mk < 0, R("market_regime_unavailable")), (~grid, family),
              (np.isnan(prev) | np.isnan(lat), R("breadth_momentum_unavailable")),
              (la > pa, R("breadth_momentum_toward_trend")), (la < pa, R("breadth_momentum_toward_range"))]
    reason = np.full(mk.shape, R("breadth_momentum_flat"), np.int64)
    for cond, code in reversed(checks):
        reason = np.where(cond, code, reason)
    allow = (reason == R("breadth_momentum_toward_trend")) | (reason == R("breadth_momentum_toward_range"))
    return allow, reason.astype(np.uint8), np.where(allow, (lat - prev) * 100, np.nan)
