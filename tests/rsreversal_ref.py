"""numpy restatement of RelativeStrengthReversalRange.signal()
(strategies/relative_strength_reversal_range.py:75-101 with regime_routing
:56-73), candle by candle on df.iloc[first:t + 1]: the oracle of the GPU
tests, pinned to what the real class did by tests/golden/rsreversal_gates.npz
(tests/test_rsreversal_ref.py).

The volume floor is Series.quantile: np.percentile(method="linear") over the
non-NaN rows of the window, +-inf kept as values, with numpy's two-sided lerp
applied also where the fraction is 0, at the quantile (q * 100) / 100, the
round trip pandas and numpy take (series_quantile). pandas' ROLLING
quantile is another function (a one-sided lerp, +-inf a missing observation):
rolling_quantile restates the staged composition for the tests that tell the
two apart.
"""

from __future__ import annotations

import numpy as np

DEFAULTS = dict(window=96, quantile=0.20, avg_return_max=-0.02, rs_min=0.05)
(EMIT, NO_FRAME, SHORT_FRAME, NO_CONTEXT, REGIME_NONE, NOT_RANGE, MARKET_NOT_WEAK, NO_FEATURES, RS_INSUFFICIENT,
 DEAD_TAPE) = range(10)
REASONS = ("emit", "no_frame", "short_frame", "market_context_unavailable", "market_regime_unavailable",
           "market_regime_not_range", "market_avg_return_not_weak_enough", "symbol_regime_unavailable",
           "symbol_rs_vs_btc_insufficient", "dead_tape")
VALUES = ("volume_floor",)
ROUTE = "range_rs_reversal"
MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")
RANGE = MARKET_REGIMES.index("RANGE")
MAX_WINDOW = 192


def quantile_parts(w, q: float):
    """(n, g, a, b): the non-NaN count of window w, the virtual index's
    fraction and the two neighbouring order statistics (NaN where n == 0)."""
    w = np.asarray(w, np.float64)
    s = np.sort(w[~np.isnan(w)])
    n = len(s)
    if n == 0:
        return 0, 0.0, np.nan, np.nan
    q = np.float64(q) * 100.0 / 100.0   # Series.quantile hands numpy the percentile q * 100; numpy divides it by 100
    vi = np.float64(n - 1) * q
    fl = np.floor(vi)
    lo = int(fl)
    return n, float(vi - fl), s[lo], s[min(lo + 1, n - 1)]


def series_quantile(w, q: float) -> float:
    """pd.Series(w).quantile(q), bit for bit."""
    n, g, a, b = quantile_parts(w, q)
    if n == 0:
        return float("nan")
    with np.errstate(invalid="ignore"):
        d = b - a
        return float(b - d * (np.float64(1.0) - g) if g >= 0.5 else a + d * g)


def rolling_quantile(w, q: float) -> float:
    """The last value of pd.Series(w).rolling(len(w), min_periods=1).quantile(q):
    +-inf is a missing observation, the lerp is one-sided."""
    w = np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        s = np.sort(w[(w - w) == 0.0])
    n = len(s)
    if n == 0:
        return float("nan")
    idx = np.float64(q) * np.float64(n - 1)
    lo = int(idx)
    if lo == idx or n == 1:
        return float(s[lo])
    return float(s[lo] + (s[lo + 1] - s[lo]) * (idx - lo))


def _rows(v, S, default):
    return np.full(S, default, np.int64) if v is None else np.asarray(v, np.int64).reshape(S)


def replay(volume, context_ok, market_regime, average_return, features_ok, rs, *, first_t=None, lens=None,
           from_t=None, floor=series_quantile, **params) -> dict:
    """status uint8 [S, T] and volume_floor [S, T]. The context arrays have 1
    or T entries, the symbol arrays are [S] or [S, T]; context_ok / features_ok
    None: present."""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    P = {**DEFAULTS, **params}
    W, q = int(P["window"]), float(P["quantile"])
    volume = np.asarray(volume, np.float64)
    S, T = volume.shape
    first, ln, frm = _rows(first_t, S, 0).clip(0, T), _rows(lens, S, T).clip(0, T), _rows(from_t, S, 0).clip(0, T)
    ctx = lambda a, dflt: np.broadcast_to(np.asarray(dflt if a is None else a).reshape(-1), (T,))   # noqa: E731
    sym = lambda a, dflt: np.broadcast_to(   # noqa: E731
        np.full(S, dflt).reshape(S, 1) if a is None else np.asarray(a).reshape(S, -1), (S, T))
    cok, mk, ar = ctx(context_ok, True).astype(bool), ctx(market_regime, 0).astype(np.int64), ctx(average_return, 0.0)
    fok, rsv = sym(features_ok, True).astype(bool), sym(rs, 0.0).astype(np.float64)
    status = np.full((S, T), NO_FRAME, np.uint8)
    vfloor = np.full((S, T), np.nan)
    for s in range(S):
        for t in range(max(int(frm[s]), int(first[s])), int(ln[s])):
            if t + 1 - first[s] < W:                       # :85
                st = SHORT_FRAME
            elif not cok[t]:                               # :61
                st = NO_CONTEXT
            elif mk[t] < 0:                                # :63
                st = REGIME_NONE
            elif mk[t] != RANGE:                           # :65
                st = NOT_RANGE
            elif ar[t] >= P["avg_return_max"]:             # :67
                st = MARKET_NOT_WEAK
            elif not fok[s, t]:                            # :69
                st = NO_FEATURES
            elif rsv[s, t] <= P["rs_min"]:                 # :71
                st = RS_INSUFFICIENT
            else:
                vfloor[s, t] = floor(volume[s, t - W + 1:t + 1], q)   # :97-98
                st = DEAD_TAPE if volume[s, t] <= vfloor[s, t] else EMIT   # :100
            status[s, t] = st
    return dict(status=status, volume_floor=vfloor)
