"""Deterministic inputs of the top-gainer fixture (tests/golden/topgainer_gates.npz).

Shared by tests/golden/make_golden_topgainer.py (which runs the REAL
reference methods on these inputs where the reference is mounted) and the
tests (which regenerate the same inputs and compare with the recorded
outputs). Only numpy's default_rng is used; the fixture stores a digest of
the inputs, so a generator drift shows up as a digest mismatch, not as a
parity failure.

The panel: 48 symbols x 700 15-minute candles of quiet seeded walks with an
injected breakout set-up every 64 candles, shaped like the reference's own
make_breakout_candles() (tests/test_top_gainer_early_momentum.py:85-155): a
gentle 5-hour rise, a +6 % hour whose last candle closes +3 % near its high on
four times the usual volume, two confirming closes, then a decay back to the
base before the next set-up's lookback begins. The set-ups cycle through
VARIANTS: clean ones, one deliberately spoiled variant per rejection of
_entry_allows and of the confirmation, and candles with zero / negative / NaN
fields and NaN / zero ATRs.
"""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 48, 700, 20261101
T0, STEP = 1_760_400_000_000, 900_000
EVENT_FIRST, EVENT_EVERY = 110, 64
K_SAMPLED = 80
VARIANTS = ("ok", "not_breaking", "below_ema", "not_green", "ok", "candle_big", "hour_big", "extension", "not_accel",
            "six_hour", "vol_low", "not_near_high", "inverted_wick", "first_fail", "second_fail", "risk",
            "zero_volume", "neg_open", "nan_close", "nan_atr", "zero_atr_conf", "nan_atr_conf", "zero_low",
            "nan_volume")
FIRST_T = {5: 99, 6: 250, 7: 37}   # rows whose first candles post_process dropped
# inverted_wick: the only way past close_not_near_high into upper_wick_too_large. range_position +
# upper_wick_fraction = (h - l) / (h - l + 1e-6), so 0.75 + 0.30 needs h - l + 1e-6 < 0: low > close > high
WICK_LOW, WICK_HIGH = 7.8e-6, 3.2e-6
# the sampled candles after a breakout b that each spoiled-candle variant needs (besides b and b + 2)
EXTRA = {"zero_volume": (5, 7), "neg_open": (6, 8), "zero_low": (7, 9), "nan_close": (8, 9, 10, 12, 16),
         "nan_volume": (5, 7, 20), "nan_atr": (5, 7), "first_fail": (1,), "second_fail": (1,)}


def events(s: int):
    """(breakout index, variant) of symbol s's injected set-ups."""
    out = []
    for j in range(64):
        b = EVENT_FIRST + EVENT_EVERY * j + s % 5
        if b >= T - 4:
            break
        out.append((b, VARIANTS[(5 * s + j) % len(VARIANTS)]))
    return out


def topgainer_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    o, h, l, c, v, qv, atr = (np.empty((S, T)) for _ in range(7))
    risk_ok = np.ones((S, T), bool)
    risk_kind = np.zeros((S, T), np.uint8)
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + s)
        scale = 10.0 ** g.uniform(-3.0, 4.0)
        r = g.normal(0.0, 0.0015, T)
        up = g.uniform(0.0, 0.0015, T)
        dn = g.uniform(0.0, 0.0015, T)
        vol = 10.0 ** g.uniform(1.0, 5.0) * np.exp(g.normal(0.0, 0.15, T))
        a_pct = g.uniform(0.004, 0.012, T)
        risk_ok[s] = g.random(T) >= 0.10
        risk_kind[s] = g.integers(0, 5, T)
        ev = events(s)
        for b, kind in ev:
            r[b - 24:b - 4] = 0.03 / 20 + g.normal(0.0, 0.0004, 20)     # a gentle 5-hour rise
            r[b - 3:b] = g.uniform(0.008, 0.012, 3)                     # the breakout hour
            r[b] = np.log(1.0 + g.uniform(0.025, 0.04))
            r[b + 1], r[b + 2] = g.uniform(0.002, 0.006), g.uniform(0.004, 0.008)
            r[b + 3:b + 15] = (-0.085 / 12 + g.normal(0.0, 0.0004, 12))[:T - (b + 3)]   # back to the base
            vol[b] *= g.uniform(3.5, 5.0)
            if kind == "below_ema":
                r[b - 50] = np.log(0.3)            # a crash 50 candles ago: ema50 still far above
            elif kind == "not_green":
                r[b - 3:b] = g.uniform(0.018, 0.022, 3)
                r[b] = np.log(1.0 + g.uniform(0.003, 0.007))
            elif kind == "candle_big":
                r[b] = np.log(1.0 + g.uniform(0.11, 0.13))
            elif kind == "hour_big":
                r[b - 3:b + 1] = g.uniform(0.055, 0.065, 4)
            elif kind == "extension":
                r[b - 90:b - 10] += 0.45 / 80
            elif kind == "not_accel":
                r[b - 8:b] = g.normal(0.0, 0.0004, 8)
                r[b - 3:b] = g.uniform(0.005, 0.007, 3)
                r[b] = np.log(1.0 + g.uniform(0.012, 0.018))
            elif kind == "six_hour":
                r[b - 24:b - 4] = -0.025 / 20 + g.normal(0.0, 0.0003, 20)
                r[b - 3:b] = g.uniform(0.011, 0.013, 3)
            elif kind == "vol_low":
                vol[b] = vol[b - 1]
            elif kind == "first_fail":
                r[b + 1] = -g.uniform(0.05, 0.07)
            elif kind == "second_fail":
                r[b + 2] = -g.uniform(0.008, 0.015)
            if kind in ("ok", "zero_atr_conf", "nan_atr_conf"):
                risk_ok[s, b + 2] = True
            elif kind == "risk":
                risk_ok[s, b + 2] = False
        cc = scale * np.exp(np.cumsum(r))
        oo = np.r_[cc[0], cc[:-1]]
        hh = np.maximum(oo, cc) * (1.0 + up)
        ll = np.minimum(oo, cc) * (1.0 - dn)
        aa = a_pct * cc
        for b, kind in ev:
            if kind == "not_breaking":
                hh[b - 10] = cc[b] * 1.03          # a wick inside the lookback
            elif kind == "not_near_high":
                hh[b] = cc[b] * 1.025
            elif kind == "inverted_wick":
                ll[b], hh[b] = cc[b] + WICK_LOW, cc[b] - WICK_HIGH
            elif kind == "zero_volume":
                vol[b + 5] = 0.0
            elif kind == "neg_open":
                oo[b + 6] = -oo[b + 6]
            elif kind == "zero_low":
                ll[b + 7] = 0.0
            elif kind == "nan_close":
                cc[b + 8] = np.nan
            elif kind == "nan_volume":
                vol[b + 5] = np.nan
            elif kind == "nan_atr":
                aa[b + 5] = np.nan
            elif kind == "zero_atr_conf":
                aa[b + 2] = 0.0
            elif kind == "nan_atr_conf":
                aa[b + 2] = np.nan
        o[s], h[s], l[s], c[s], v[s], atr[s] = oo, hh, ll, cc, vol, aa
        qv[s] = vol * np.where(np.isnan(cc), scale, cc) * g.uniform(0.98, 1.02, T)
    first = np.zeros(S, np.int64)
    for s, f in FIRST_T.items():
        first[s] = f
    ts = np.broadcast_to(T0 + STEP * np.arange(T, dtype=np.int64), (S, T)).copy()
    return dict(open=o, high=h, low=l, close=c, volume=v, quote_volume=qv, atr=atr, open_time=ts, first_t=first,
                risk_ok=risk_ok, risk_kind=risk_kind)


def sample_positions(seed: int = SEED) -> np.ndarray:
    """[S, K_SAMPLED] sorted candle indices per symbol at which the outputs
    are recorded: every set-up's breakout candle and second confirmation, the
    candles a spoiled field touches, the min-history edges, the first and the
    last rows, and random positions."""
    g = np.random.default_rng(seed + 77)
    rows = []
    for s in range(S):
        f = FIRST_T.get(s, 0)
        pos = {0, 1, f + 54, f + 55, f + 56, f + 57, f + 58, T - 3, T - 2, T - 1}
        for b, kind in events(s):
            pos.update((b, b + 2))
            pos.update(b + d for d in EXTRA.get(kind, ()))
        pos = sorted(p for p in pos if 0 <= p < T)
        assert len(pos) <= K_SAMPLED, (s, len(pos))
        rest = np.setdiff1d(np.arange(T), pos)
        rows.append(np.sort(np.r_[pos, g.choice(rest, K_SAMPLED - len(pos), replace=False)]))
    return np.array(rows, dtype=np.int64)


# ---- stand-in contexts: what a refused risk_ok candle looks like, and the _risk_profile_allows grid -----------
BENIGN = dict(context_ok=True, stress=0.1, long_score=0.64, short_score=0.2, regime_score=0.1, btc_return=0.005,
              features_ok=True, rs=0.04, atr_pct=0.025, regime="TREND_UP", transition="BREAKOUT_UP", trend=0.05)
REFUSALS = (dict(stress=0.9), dict(context_ok=False), dict(features_ok=False), dict(rs=0.0),
            dict(transition="VOLATILITY_EXPANSION"))   # risk_kind's index


def risk_case_at(risk_ok: bool, kind: int) -> dict:
    return dict(BENIGN) if risk_ok else {**BENIGN, **REFUSALS[int(kind)]}


def risk_cases(seed: int = SEED) -> list[dict]:
    """A few hundred stand-in context / feature combinations: every check of
    _risk_profile_allows refused alone on a benign base, then seeded mixtures
    (no value on a threshold's tie except the documented ones: stress 0.25
    refuses, rs 0.03 refuses, atr_pct 0.06 allows)."""
    g = np.random.default_rng(seed + 5)
    regimes = ("TREND_UP", "TREND_DOWN", "TREND_DOWN", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL", None)
    transitions = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                   "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL", None)
    single = [dict(context_ok=False), dict(stress=0.25), dict(stress=0.4), dict(short_score=0.8),
              dict(short_score=0.64 + 0.16), dict(regime_score=-0.3, btc_return=-0.01),
              dict(regime_score=-0.3, btc_return=0.01), dict(regime_score=-0.1, btc_return=-0.01),
              dict(features_ok=False), dict(rs=0.03), dict(rs=0.0), dict(rs=-0.2), dict(atr_pct=0.061),
              dict(atr_pct=0.06), dict(transition="BREAKDOWN"), dict(transition="ENTERED_TREND_DOWN"),
              dict(transition="VOLATILITY_EXPANSION"), dict(transition=None), dict(regime="TREND_DOWN", trend=-0.05),
              dict(regime="TREND_DOWN", trend=0.05), dict(regime=None, trend=-0.05), {}]
    out = [{**BENIGN, **d} for d in single]
    for _ in range(400 - len(out)):
        out.append(dict(
            context_ok=bool(g.random() < 0.93), stress=float(g.choice([0.05, 0.1, 0.15, 0.2, 0.24, 0.26, 0.5])),
            long_score=float(g.uniform(0.1, 1.0)), short_score=float(g.uniform(0.0, 0.6)),
            regime_score=float(g.choice([-0.5, -0.25, -0.15, 0.0, 0.1, 0.3])),
            btc_return=float(g.choice([-0.02, -0.001, 0.001, 0.02])), features_ok=bool(g.random() < 0.93),
            rs=float(g.choice([-0.05, 0.029, 0.031, 0.05, 0.08, 0.2])),
            atr_pct=float(g.choice([0.01, 0.02, 0.03, 0.059, 0.0601, 0.09])),
            regime=regimes[int(g.integers(0, len(regimes)))],
            transition=transitions[int(g.integers(0, len(transitions)))],
            trend=float(g.choice([-0.1, -0.001, 0.001, 0.1]))))
    return out


def digest(panel: dict[str, np.ndarray]) -> str:
    hsh = hashlib.sha256()
    for f in sorted(panel):
        hsh.update(f.encode())
        hsh.update(np.ascontiguousarray(panel[f]).tobytes())
    return hsh.hexdigest()
