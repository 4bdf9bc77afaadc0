"""The panel of the per-symbol regime fixture (regime_panel.npz) and the
near-tie test of its cells — numpy only, so the fixture's generator and the
tests rebuild the same candles.

64 symbols x 120 timestamps of seeded walks with the fresh fixture's absences
(make_golden_fresh.py):

  rows 1-8    late listings, first candles at t = 5 .. 90
  rows 9-12   one halt of 10-40 candles each, then they resume
  rows 13-18  scattered single missing candles
  row 19      delists at t = 60
  row 20      never present
  row 21      first candle at the last timestamp
  row 0       BTC, absent at t = 70, 71, 72
  rows 40-63  24 symbols absent together over t = 100 .. 107 (18 of them from
              t = 95): the coverage-gated stretch
and two groups that reach the regimes a calm walk never does:
  rows 22-27  per-candle sigma 0.03 (VOLATILE, and back)
  rows 28-33  drift +-0.004 flipping sign every 30 candles, sigma 0.003
              (TREND_UP / TREND_DOWN and the transitions between them)
"""

from __future__ import annotations

import numpy as np

S, T, MAX_BARS, SEED = 64, 120, 30, 20261024
BTC = 0
VOLATILE_ROWS = range(22, 28)
FLIP_ROWS = range(28, 34)
CUT_EPS = 1e-6


def build_panel():
    """(open, high, low, close, present), each [S, T]."""
    rng = np.random.default_rng(SEED)
    ret = rng.normal(0.0002, 0.006, (S, T))
    for s in VOLATILE_ROWS:
        ret[s] = rng.normal(0.0, 0.03, T)
    sign = np.where((np.arange(T) // 30) % 2 == 0, 1.0, -1.0)
    for i, s in enumerate(FLIP_ROWS):
        ret[s] = (sign if i % 2 == 0 else -sign) * 0.004 + rng.normal(0.0, 0.003, T)
    scale = 10 ** rng.uniform(-2, 3, S)
    scale[BTC] = 60_000.0
    c = scale[:, None] * np.exp(np.cumsum(ret, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * (1 + rng.uniform(0, 0.003, (S, T)))
    l = np.minimum(o, c) * (1 - rng.uniform(0, 0.003, (S, T)))
    present = np.ones((S, T), dtype=bool)
    for i, t0 in enumerate((5, 17, 29, 41, 53, 65, 77, 90)):       # late listings
        present[1 + i, :t0] = False
    for i, (a, n) in enumerate(((20, 10), (35, 25), (40, 40), (70, 15))):   # halts
        present[9 + i, a:a + n] = False
    for s in range(13, 19):                                          # single missing candles
        present[s, rng.choice(np.arange(3, 93), 5, replace=False)] = False
    present[19, 60:] = False                                         # delisting
    present[20, :] = False                                           # never present
    present[21, :T - 1] = False                                      # listed at the last timestamp
    present[BTC, 70:73] = False                                      # BTC gap
    present[40:64, 100:108] = False                                  # 24 absent together
    present[46:64, 95:100] = False
    return o, h, l, c, present


def timestamps() -> np.ndarray:
    return 1_760_200_000_000 + 900_000 * np.arange(T, dtype=np.int64)


def micro_scores(trend, above20, above50, rs, bb_width, atr_pct):
    """The four scores of _annotate_symbol_regime (regime_transitions.py:167-195), element-wise."""
    trend, rs = np.asarray(trend, np.float64), np.asarray(rs, np.float64)
    bbw, atr = np.asarray(bb_width, np.float64), np.asarray(atr_pct, np.float64)
    a20, a50 = np.asarray(above20, np.float64), np.asarray(above50, np.float64)
    clamp01 = lambda x: np.maximum(0.0, np.minimum(1.0, x))  # noqa: E731
    nn = lambda x: np.maximum(0.0, x)  # noqa: E731
    up = clamp01(0.45 * nn(trend * 30.0) + 0.2 * a20 + 0.15 * a50 + 0.2 * nn(rs * 20.0))
    down = clamp01(0.45 * nn(-trend * 30.0) + 0.2 * (1.0 - a20) + 0.15 * (1.0 - a50) + 0.2 * nn(-rs * 20.0))
    rng = clamp01(0.38 * (1.0 - np.minimum(np.abs(trend) * 30.0, 1.0)) + 0.34 * (1.0 - np.minimum(bbw / 0.08, 1.0))
                  + 0.28 * (1.0 - np.minimum(atr / 0.04, 1.0)))
    vol = clamp01(0.55 * np.minimum(atr / 0.05, 1.0) + 0.45 * np.minimum(bbw / 0.12, 1.0))
    return up, down, rng, vol


def near_cut(trend, above20, above50, rs, bb_width, atr_pct, return_pct, close=None, ema20=None, ema50=None,
             eps: float = CUT_EPS):
    """True where a cell lies within eps of a cut point of the micro regime
    (0.72, 0.015, 0.52, the two 0.1 gaps, 0.5) or, given close and the EMAs,
    within eps (relative) of close == ema20 / ema50: there a 1e-9 difference
    in the features may change a label."""
    up, down, rng, vol = micro_scores(trend, above20, above50, rs, bb_width, atr_pct)
    ret = np.abs(np.asarray(return_pct, np.float64))
    near = (np.abs(vol - 0.72) <= eps) | (np.abs(ret - 0.015) <= eps) | (np.abs(up - 0.52) <= eps)
    near |= (np.abs(down - 0.52) <= eps) | (np.abs(up - (down + 0.1)) <= eps) | (np.abs(down - (up + 0.1)) <= eps)
    near |= np.abs(rng - 0.5) <= eps
    if close is not None:
        cl = np.asarray(close, np.float64)
        for e in (ema20, ema50):
            near |= np.abs(cl - np.asarray(e, np.float64)) <= eps * np.abs(cl)
    return near
