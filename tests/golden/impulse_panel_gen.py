"""Deterministic inputs of the impulse-rider / ladder-stability fixture
(tests/golden/impulse_gates.npz).

Shared by tests/golden/make_golden_impulse.py (which runs the REAL reference
methods on these inputs where the reference is mounted) and the tests (which
regenerate the same inputs and compare with the recorded outputs). Only
numpy's default_rng is used; the fixture stores a digest of the inputs, so a
generator drift shows up as a digest mismatch, not as a parity failure.

The panel: 48 symbols x 600 15-minute candles of seeded random walks with an
injected event every 28 candles, shaped like the reference's own
make_candles() (tests/test_relative_strength_impulse_rider.py:17-34): four
flat-ish bars, a +5-18 % trigger hour, a confirmation closing in the top 30 %
of its range, ATR 1-5 % of price, the benchmark flat across the hour. The
events cycle through VARIANTS: clean ones and one deliberately spoiled
variant per rejection of RelativeStrengthImpulseRider._features.
"""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 48, 600, 20261021
T0, STEP = 1_760_400_000_000, 900_000
EVENT_FIRST, EVENT_EVERY = 40, 28
K_SAMPLED = 80
VARIANTS = ("ok", "big", "ok", "small", "cross", "btc_hi", "ok", "rs_low", "atr_hi", "no_hold", "conf_neg",
            "loc_low", "ok", "flat", "nan_atr", "zero_anchor", "neg_anchor", "nan_anchor", "btc_hole", "zero_open")
FIRST_T = {5: 99, 6: 120}        # rows whose first candles post_process dropped
SHIFTED = 7                      # a symbol on a grid shifted by half a step: no benchmark matches
BENCH_A_START = 28               # benchmark A begins at the panel's candle 28 (matches at position < 4)
MIN_IMPULSE_GRID = (-0.02, -0.012, -0.007, -0.003, 0.0, 0.003, 0.007, 0.012, 0.02, 0.05)


def events(s: int):
    """(trigger index, variant) of symbol s's injected events."""
    out = []
    for j in range(64):
        tr = EVENT_FIRST + EVENT_EVERY * j + s % 7
        if tr >= T - 8:
            break
        v = VARIANTS[(s + 3 * j) % len(VARIANTS)]
        if v in ("btc_hi", "btc_hole") and s >= 12:   # these change the shared benchmark: a few symbols only
            v = "ok"
        out.append((tr, v))
    return out


def impulse_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    o, h, l, c, atr = (np.empty((S, T)) for _ in range(5))
    ts = np.empty((S, T), np.int64)
    bench_r = np.random.default_rng(seed + 999).normal(0.0, 0.0006, T + 10)   # flat-ish benchmark
    holes, dup_at = [], None
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + s)
        scale = 10.0 ** g.uniform(-3.0, 4.0)
        r = g.normal(0.0, 0.005, T)
        up = g.uniform(0.0, 0.003, T)
        dn = g.uniform(0.0, 0.003, T)
        a_pct = np.full(T, g.uniform(0.01, 0.05))
        ev = events(s)
        for tr, v in ev:
            cf = tr + 1
            r[tr - 5: tr] = g.normal(0.0, 0.0008, 5)            # four flat-ish bars before the hour's last candle
            imp = g.uniform(0.085, 0.17)                        # with a flat benchmark: relative strength >= 0.08
            if v == "big":
                imp = g.uniform(0.19, 0.30)
            elif v == "small":
                imp = g.uniform(0.01, 0.045)
            elif v == "rs_low":
                imp = g.uniform(0.052, 0.075)
            elif v == "cross":
                r[tr - 1] = np.log(1.0 + g.uniform(0.055, 0.07))   # the hour before already crossed 5 %
                imp = g.uniform(0.06, 0.09)
            r[tr] = np.log(1.0 + imp) - (r[tr - 3] + r[tr - 2] + r[tr - 1])
            r[cf] = g.uniform(0.001, 0.008) if v != "no_hold" else -g.uniform(0.004, 0.01)
            if v == "btc_hi":
                bench_r[tr] = np.log(1.0 + g.uniform(0.015, 0.03))
            if v == "btc_hole":
                holes.append(tr)
            if v == "ok" and dup_at is None and s == 3:
                dup_at = tr
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + up)
        ll = np.minimum(oo, cc) * (1.0 - dn)
        for tr, v in ev:
            cf = tr + 1
            # the confirmation closes in the top of its range (spoiled variants below)
            hh[cf] = cc[cf] * 1.0005
            ll[cf] = min(oo[cf], cc[cf]) * 0.998
            if v == "conf_neg":                 # closes above the trigger close but below its own open
                oo[cf] = cc[cf] * 1.004
                hh[cf] = oo[cf] * 1.0005
            elif v == "loc_low":
                hh[cf] = cc[cf] * 1.03
            elif v == "flat":
                hh[cf] = ll[cf] = cc[cf]
            elif v == "atr_hi":
                a_pct[tr] = g.uniform(0.065, 0.08)
            elif v == "nan_atr":
                a_pct[tr] = np.nan
            elif v == "zero_open":
                oo[tr] = 0.0
            elif v == "zero_anchor":
                cc[tr - 4] = 0.0
            elif v == "neg_anchor":
                cc[tr - 5] = -cc[tr - 5]
            elif v == "nan_anchor":
                cc[tr - 4] = np.nan
        o[s], h[s], l[s], c[s] = oo, hh, ll, cc
        atr[s] = a_pct * np.abs(np.where(np.isnan(cc), 1.0, cc))
        ts[s] = T0 + STEP * np.arange(T) + (STEP // 2 if s == SHIFTED else 0)
    first = np.zeros(S, np.int64)
    for s, f in FIRST_T.items():
        first[s] = f
    bench = 60000.0 * np.exp(np.cumsum(bench_r))
    grid = T0 + STEP * np.arange(T + 10, dtype=np.int64)
    # benchmark A: a regular grid from candle 28, ten rows past the panel's end
    a_ts, a_close = grid[BENCH_A_START:].copy(), bench[BENCH_A_START:].copy()
    # benchmark B: the panel's span with rows missing (the btc_hole events and three more), one time held
    # twice with different closes, and off-grid rows in between (an irregular grid; the anchor is positional)
    g = np.random.default_rng(seed + 555)
    keep = np.ones(T, bool)
    keep[sorted(set(holes))] = False
    keep[g.choice(np.arange(60, T - 5), 3, replace=False)] = False
    b_ts, b_close = list(grid[:T][keep]), list(bench[:T][keep])
    for t_extra in sorted(g.choice(np.arange(50, T - 5), 9, replace=False)):
        b_ts.append(int(grid[t_extra]) + 300_000)
        b_close.append(float(bench[t_extra]) * 1.0007)
    if dup_at is not None and keep[dup_at]:
        b_ts.append(int(grid[dup_at]))            # sorts after the first copy (stable): the later row
        b_close.append(float(bench[dup_at]) * 0.97)
    order = np.argsort(np.array(b_ts, np.int64), kind="stable")
    b_ts, b_close = np.array(b_ts, np.int64)[order], np.array(b_close)[order]
    return dict(open=o, high=h, low=l, close=c, atr=atr, open_time=ts, first_t=first, bench_a_ts=a_ts,
                bench_a_close=a_close, bench_b_ts=b_ts, bench_b_close=b_close)


def sample_positions(seed: int = SEED) -> np.ndarray:
    """[S, K_SAMPLED] sorted candle indices per symbol at which the gate's
    outputs are recorded: every event's confirmation candle, the candles
    around a spoiled anchor, the min-history edge, benchmark A's first rows,
    the last rows, and random positions."""
    g = np.random.default_rng(seed + 77)
    rows = []
    for s in range(S):
        f = FIRST_T.get(s, 0)
        pos = {0, 1, f + 18, f + 19, f + 20, f + 24, T - 2, T - 1, BENCH_A_START, BENCH_A_START + 1,
               BENCH_A_START + 4, BENCH_A_START + 5}
        for tr, v in events(s):
            pos.add(tr + 1)
            if v.endswith("_anchor"):
                pos.update((tr - 4, tr - 3, tr - 2, tr + 2))
        pos = sorted(p for p in pos if 0 <= p < T)[:K_SAMPLED]
        rest = np.setdiff1d(np.arange(T), pos)
        rows.append(np.sort(np.r_[pos, g.choice(rest, K_SAMPLED - len(pos), replace=False)]))
    return np.array(rows, dtype=np.int64)


def bb_rows(panel: dict[str, np.ndarray]) -> tuple[np.ndarray, np.ndarray]:
    """(closes [R, T], first_t [R]) behind the Bollinger columns of the
    ladder-stability fixture: ten panel rows (their NaN / zero / negative
    closes included), a row with constant stretches (upper == lower), a row
    that goes negative (bb_mid <= 0) and a row with first_t = 99."""
    c = panel["close"][:10].copy()
    flat = panel["close"][20].copy()
    flat[200:260] = flat[200]
    flat[400:419] = flat[400]       # one short of a full window of equal closes
    neg = panel["close"][21].copy()
    neg[300:340] = -neg[300:340]
    late = panel["close"][22].copy()
    closes = np.vstack([c, flat, neg, late])
    first = np.zeros(len(closes), np.int64)
    first[-1] = 99
    first[5], first[6] = FIRST_T[5], FIRST_T[6]
    return closes, first


def digest(panel: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for f in sorted(panel):
        h.update(f.encode())
        h.update(np.ascontiguousarray(panel[f]).tobytes())
    return h.hexdigest()
