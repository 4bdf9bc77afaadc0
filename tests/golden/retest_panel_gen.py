"""Deterministic inputs of the gradual-gainer retest fixture
(tests/golden/retest_gates.npz).

Shared by tests/golden/make_golden_retest.py (which drives the REAL
GradualGainerRetest.signal() over these inputs where the reference is mounted)
and the tests (which regenerate the same inputs and compare with the recorded
outputs). Only numpy's default_rng is used; the fixture stores a digest of the
inputs, so a generator drift shows up as a digest mismatch, not as a parity
failure.

The panel: 32 rows x 700 15-minute candles against a flat-ish benchmark on the
full grid, and a seeded risk mask (what the fixture run's _risk_allows returns
per candle). Row kinds (KINDS):

  walk     a random walk with an upward burst about every 60 candles: watches
           that become candidates within a few candles;
  decline  an 8-candle burst, then a steady 48-candle decline of small red
           candles: the watch set near the top fails the pullback test until
           it expires;
  rise     stretches of sustained drift during which the risk mask is False
           throughout: the watch can only be risk-blocked, expires 8 hours
           later, and the next leader candle — often the expiring one itself —
           sets it again;
  late     walks whose frame starts at candle 99 / 120 (first_t);
  nan      a walk with 4 % of its highs and lows missing and, across each
           burst's start, a run of 15 missing highs (a level that is NaN);
  gaps     (GAP_ROWS: some decline rows and three walks) rows with dropped
           candles: their open times jump, so 8 hours are fewer than 32 rows.

Rows with dropped candles are shorter than T (lens); the columns past a row's
length hold NaN and ascending pad times.
"""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 32, 700, 20261023
T0, STEP = 1_760_400_000_000, 900_000
KINDS = ("walk",) * 12 + ("decline",) * 8 + ("rise",) * 6 + ("late",) * 2 + ("nan",) + ("walk",) * 3
FIRST_T = {26: 99, 27: 120}
GAP_ROWS = (16, 17, 18, 19, 29, 30, 31)


def _risk_mask(g, n: int, p_false: float = 0.3, mean_run: float = 4.0) -> np.ndarray:
    """Runs of True / False (geometric lengths): False about p_false of the time."""
    out = np.ones(n, bool)
    t = 0
    while t < n:
        run_true = int(g.geometric(p_false / (mean_run * (1.0 - p_false))))
        t += run_true
        run_false = int(g.geometric(1.0 / mean_run))
        out[t:t + run_false] = False
        t += run_false
    return out


def retest_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    o, h, l, c = (np.full((S, T), np.nan) for _ in range(4))
    ts = np.empty((S, T), np.int64)
    risk = np.ones((S, T), bool)
    lens = np.full(S, T, np.int64)
    first = np.zeros(S, np.int64)
    for s, f in FIRST_T.items():
        first[s] = f
    grid = T0 + STEP * np.arange(T + 40, dtype=np.int64)
    gb = np.random.default_rng(seed + 999)
    btc_close = 60000.0 * np.exp(np.cumsum(gb.normal(0.0, 0.001, T + 40)))
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + s)
        kind = KINDS[s]
        scale = 10.0 ** g.uniform(-2.0, 3.0)
        r = g.normal(0.0, 0.005, T)
        up = g.uniform(0.0, 0.004, T)     # upper wick
        dn = g.uniform(0.0, 0.004, T)     # lower wick
        ok = _risk_mask(g, T)
        nan_hi = np.zeros(T, bool)
        if kind in ("walk", "late", "nan"):
            b = 30 + int(g.integers(0, 20))
            while b < T - 12:
                n = int(g.integers(6, 11))
                r[b:b + n] = g.normal(0.008, 0.003, n)
                if kind == "nan":
                    nan_hi[max(b - 8, 0):b + 7] = True
                b += 45 + int(g.integers(0, 30))
        elif kind == "decline":
            b = 40 + int(g.integers(0, 16))
            while b < T - 60:
                r[b:b + 8] = g.normal(0.012, 0.002, 8)
                r[b + 8:b + 56] = -np.abs(g.normal(0.0025, 0.0008, 48))
                up[b + 8:b + 56] *= 0.3
                b += 56 + int(g.integers(0, 8))
        elif kind == "rise":
            b = 60 + int(g.integers(0, 20))
            while b < T - 130:
                n = 110 + int(g.integers(0, 20))
                r[b:b + n] = g.normal(0.003, 0.004, n)
                ok[b + 20:b + n + 40] = False
                b += n + 60 + int(g.integers(0, 20))
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + up)
        ll = np.minimum(oo, cc) * (1.0 - dn)
        if kind == "nan":
            holes = g.random((2, T)) < 0.04
            hh[holes[0] | nan_hi] = np.nan
            ll[holes[1]] = np.nan
        keep = np.ones(T, bool)
        if s in GAP_ROWS:   # dropped candles: singles and short runs
            for start in g.choice(np.arange(30, T - 10), 40, replace=False):
                keep[start:start + int(g.integers(1, 5))] = False
        n = int(keep.sum())
        lens[s] = n
        o[s, :n], h[s, :n], l[s, :n], c[s, :n] = oo[keep], hh[keep], ll[keep], cc[keep]
        ts[s, :n] = grid[:T][keep]
        ts[s, n:] = ts[s, n - 1] + STEP * np.arange(1, T - n + 1)
        risk[s, :n] = ok[keep]
    return dict(open=o, high=h, low=l, close=c, open_time=ts, risk_ok=risk, lens=lens, first_t=first,
                btc_time=grid, btc_close=btc_close)


def risk_cases(seed: int = SEED + 5):
    """A seeded grid of stand-in contexts for _risk_allows: every value set
    holds the method's thresholds, their neighbours and NaN."""
    regimes = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
    transitions = (None, "VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                   "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
    g = np.random.default_rng(seed)
    pick = lambda xs: xs[int(g.integers(0, len(xs)))]   # noqa: E731
    cases = []
    for i in range(480):
        cases.append(dict(
            context_ok=g.random() > 0.06, features_ok=g.random() > 0.08,
            stress=pick((0.0, 0.1, 0.2, 0.24999, 0.25, 0.3, float("nan"))) if g.random() > 0.4 else 0.1,
            regime_score=pick((-0.5, -0.2000001, -0.2, -0.1, 0.3, float("nan"))),
            btc_return=pick((-0.02, -1e-9, 0.0, 0.01, float("nan"))),
            atr_pct=pick((0.01, 0.0599, 0.06, 0.0601, 0.2, float("nan"))) if g.random() > 0.4 else 0.02,
            regime=pick(regimes), transition=pick(transitions),
            trend=pick((-0.3, -1e-12, 0.0, 0.2, float("nan")))))
    return cases


def digest(panel: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for f in sorted(panel):
        h.update(f.encode())
        h.update(np.ascontiguousarray(panel[f]).tobytes())
    return h.hexdigest()
