"""Deterministic inputs of the liquidation-sweep fixture (tests/golden/sweep_gates.npz).

Shared by tests/golden/make_golden_sweep.py (which drives the REAL
LiquidationSweepPump.signal() over these inputs where the reference is
mounted) and the tests (which regenerate the same inputs and compare with the
recorded outputs). Only numpy's default_rng is used; the fixture stores a
digest of the inputs.

The panel: 16 symbols x 160 15-minute candles on one open-time grid, plus the
benchmark (BTC) series. Quiet seeded walks with a volume-and-price impulse
every 7 candles from candle 74 on, the rows' impulses aligned in four column
groups so that a candle time holds several candidates:

  rows 0-5, 9-12   impulse rows. The impulses cycle through VARIANTS: clean
                   ones and one spoiled variant per point-wise check of
                   _is_candidate (too large for its ATR, a wick above in the
                   compression window, a close far from the high, no volume).
                   Rows 1 and 3 are copies of rows 0 and 2 (bit-equal scores:
                   the selector's symbol tie-break decides), rows 11 / 12
                   start late (FIRST_T), rows 9 / 10 end early (LENS).
  row 7            falls 0.8 % a candle until candle 72, then turns: its
                   impulses (from candle 96) meet trend_score <= 0.
  rows 6, 8        a 24-candle saw-tooth (a twelve-candle rally, a four-candle
                   dip, six flat candles, a small impulse): ema20 > ema50 but
                   the close is still under ema20.
  rows 13-15       slowly falling closes with one small uptick every five
                   candles, timed so that at the impulse fewer than ten of the
                   48 earlier pump scores are positive: score_threshold == 0.

The benchmark falls over candles 44-62 and recovers (btc_trend_score < 0 with
btc_momentum_3 > 0 for some twenty candles), jumps 2 % at BTC_JUMPS (relative
strength <= 0 for three candles) and drops at BTC_DROPS (btc_momentum_3 < 0).

NAMES are chosen so that Python's str order differs from the row order
("B10USDTM" < "B9USDTM"). route_ok / route_kind: the seeded routing verdict
per (symbol, candle) and the stand-in refusal it is made of (REFUSALS);
routing_cases(): the grid long_entry_routing is recorded on.
"""

from __future__ import annotations

import hashlib

import numpy as np

S, T, SEED = 16, 160, 20261020
T0, STEP = 1_760_400_000_000, 900_000
NAMES = tuple(f"B{n}USDTM" for n in (7, 8, 9, 10, 11, 12, 3, 4, 5, 6, 13, 14, 15, 16, 1, 2))
FIRST_T = {11: 30, 12: 50}
LENS = {9: 150, 10: 141}
TWINS = {1: 0, 3: 2}
OFFSET = {0: 0, 1: 0, 10: 0, 2: 2, 3: 2, 11: 2, 4: 4, 5: 4, 12: 4, 7: 6, 9: 6}
SAWTOOTH = {6: 90, 8: 78}   # row -> its first impulse; one every 24 candles
EVENT_FIRST, EVENT_EVERY = 74, 7
VARIANTS = ("ok", "close_loc", "matr", "ok", "prior_high", "ok", "ok", "ok", "ok", "volume")
BTC_FALL, BTC_JUMPS, BTC_DROPS = (44, 62), (96, 128), (112, 144)
THRESHOLD_ROWS = {13: (100, 153), 14: (102, 155), 15: (104, 157)}
REFUSALS = ("no_context", "stress", "not_washed_out", "not_recovering", "two_values", "no_features", "trend_not_up")
BENIGN = dict(context_ok=True, stress=0.1, breadth=(-0.52, -0.46, -0.42), features_ok=True, trend=0.02)


def zone_columns() -> set[int]:
    """Columns whose benchmark decides the outcome: the impulses there stay clean."""
    z = set(range(EVENT_FIRST, 88))
    for b in BTC_JUMPS + BTC_DROPS:
        z |= {b, b + 1, b + 2}
    return z


def events(s: int):
    """(impulse candle, variant) of an impulse row."""
    zone = zone_columns()
    out = []
    for k in range(64):
        b = EVENT_FIRST + OFFSET[s] + EVENT_EVERY * k
        if b >= T - 2:
            break
        out.append((b, "ok" if b in zone else VARIANTS[(k + 3 * s) % len(VARIANTS)]))
    return out


def _candles(c, g, wick=(0.001, 0.003)):
    o = np.r_[c[0], c[:-1]]
    h = np.maximum(o, c) * (1.0 + g.uniform(*wick, len(c)))
    l = np.minimum(o, c) * (1.0 - g.uniform(*wick, len(c)))
    return o, h, l


def _impulse_row(s: int, g):
    falling = s == 7
    r = (-0.0005 if falling else 0.0005) + g.normal(0.0, 0.001, T)
    if falling:
        r[:72] = -0.008 + g.normal(0.0, 0.0003, 72)
    base = 10.0 ** g.uniform(2.0, 4.0)
    vol = base * np.exp(g.normal(0.0, 0.15, T))
    size = g.uniform(0.011, 0.014) * (0.85 if s in (10, 11) else 1.0)
    ev = [(b, "ok" if falling else kind) for b, kind in events(s) if not falling or b >= 96]
    for b, kind in ev:
        imp = {"matr": 0.045, "volume": 0.016}.get(kind, size)
        r[b] = np.log1p(imp)
        r[b - 1] = -0.0005
        vol[b] = base * (0.8 if kind == "volume" else 4.0)
    c = 10.0 ** g.uniform(-2.0, 3.0) * np.exp(np.cumsum(r))
    o, h, l = _candles(c, g)
    for b, kind in ev:
        if kind == "prior_high":
            h[b - 3] = c[b] * 1.008
        elif kind == "close_loc":
            h[b] = c[b] * 1.012
    return o, h, l, c, vol


def _sawtooth_row(s: int, g):
    """Per 24 candles: a twelve-candle rally, a four-candle dip, six flat candles, the impulse."""
    r = g.normal(0.0, 0.0004, T)
    base = 10.0 ** g.uniform(2.0, 4.0)
    vol = base * np.exp(g.normal(0.0, 0.15, T))
    for b in range(SAWTOOTH[s], T - 2, 24):
        r[b] = np.log1p(0.009)
        vol[b] = base * 4.0
        r[b - 23:b - 10] += 0.007
        r[b - 10:b - 6] -= 0.0175
    c = 10.0 ** g.uniform(-1.0, 2.0) * np.exp(np.cumsum(r))
    return (*_candles(c, g, (0.0005, 0.0015)), c, vol)


def _threshold_row(s: int, g):
    """Closes fall 0.005 % a candle; an uptick of 0.1 % (undone on the next
    candle) every five candles from b - 49 to b - 4 is the only positive
    momentum_3, so at the impulse b the 48 scores before it hold nine
    positive ones (threshold 0) and the 48 before b - 1 ten (threshold > 0)."""
    r = np.full(T, -0.00005)
    base = 10.0 ** g.uniform(2.0, 4.0)
    vol = base * np.exp(g.normal(0.0, 0.05, T))
    for b in THRESHOLD_ROWS[s]:
        for j in range(b - 49, b - 3, 5):
            r[j], r[j + 1] = 0.001, -0.001
        r[b] = np.log1p(0.04)
        vol[b] = base * 4.0
    c = 10.0 ** g.uniform(0.0, 2.0) * np.exp(np.cumsum(r))
    o = np.r_[c[0], c[:-1]]
    h, l = np.maximum(o, c) * 1.0075, np.minimum(o, c) * 0.9925
    for b in THRESHOLD_ROWS[s]:
        h[b] = c[b] * 1.002
    return o, h, l, c, vol


def benchmark(seed: int = SEED) -> np.ndarray:
    g = np.random.default_rng(seed * 1000 + 999)
    r = 0.0004 + g.normal(0.0, 0.0001, T)
    r[BTC_FALL[0]:BTC_FALL[1]] = -0.002
    r[BTC_FALL[1]:80] = 0.0015
    for b in BTC_JUMPS:
        r[b] = 0.02
    for b in BTC_DROPS:
        r[b] = -0.008
    return 60_000.0 * np.exp(np.cumsum(r))


def sweep_panel(seed: int = SEED) -> dict[str, np.ndarray]:
    o, h, l, c, v = (np.empty((S, T)) for _ in range(5))
    for s in range(S):
        g = np.random.default_rng(seed * 1000 + TWINS.get(s, s))
        if s in THRESHOLD_ROWS:
            row = _threshold_row(s, g)
        elif s in SAWTOOTH:
            row = _sawtooth_row(s, g)
        else:
            row = _impulse_row(TWINS.get(s, s), g)
        o[s], h[s], l[s], c[s], v[s] = row
    g = np.random.default_rng(seed * 1000 + 998)
    route_ok = g.random((S, T)) >= 0.15
    route_kind = g.integers(0, len(REFUSALS), (S, T)).astype(np.uint8)
    order = np.stack([np.random.default_rng(seed * 1000 + 500 + t).permutation(S) for t in range(T)])
    return dict(open=o, high=h, low=l, close=c, volume=v, btc_close=benchmark(seed),
                open_time=T0 + STEP * np.arange(T, dtype=np.int64),
                first_t=np.array([FIRST_T.get(s, 0) for s in range(S)], np.int64),
                lens=np.array([LENS.get(s, T) for s in range(S)], np.int64),
                route_ok=route_ok, route_kind=route_kind, order=order.astype(np.int64))


def route_case_at(ok: bool, kind: int) -> dict:
    """The stand-in context / features a cell's routing verdict is made of."""
    case = dict(BENIGN)
    if ok:
        return case
    name = REFUSALS[int(kind)]
    if name == "no_context":
        case["context_ok"] = False
    elif name == "stress":
        case["stress"] = 0.35
    elif name == "not_washed_out":
        case["breadth"] = (-0.30, -0.25, -0.19)
    elif name == "not_recovering":
        case["breadth"] = (-0.44, -0.46, -0.43)
    elif name == "two_values":
        case["breadth"] = (-0.52, -0.42)
    elif name == "no_features":
        case["features_ok"] = False
    else:
        case["trend"] = 0.0
    return case


def routing_cases(seed: int = SEED, n: int = 160) -> list[dict]:
    """Seeded stand-ins for long_entry_routing: every refusal and the
    accepting route, None context, None features, breadth series of one
    (the context's own advancers - decliners), two, three and four values."""
    g = np.random.default_rng(seed * 1000 + 997)
    cases = []
    for i in range(n):
        nb = (3, 3, 4, 3, 3, 4, 3, 2, 3, 1)[i % 10]
        last = float(g.choice([-0.6, -0.45, -0.3, -0.21, -0.25, -0.15]))
        rec = float(g.choice([0.1, 0.05, 0.021, 0.03, 0.04, 0.015]))
        series = [last - rec - 0.01, last - rec, last - 0.5 * rec, last][-nb:] if nb > 1 else [last]
        cases.append(dict(context_ok=bool(g.random() >= 0.1), stress=float(g.choice([0.05, 0.1, 0.2, 0.3, 0.34, 0.36])),
                          breadth=tuple(series), btc_momentum=float(g.choice([0.004, 0.001, -0.002, 0.0, 0.01])),
                          features_ok=bool(g.random() >= 0.15), trend=float(g.choice([0.03, 0.01, -0.01, 0.0, 0.02]))))
    return cases


def breadth_inputs(case: dict) -> tuple[float, float]:
    """(latest breadth, recovery; NaN = the method's None) of a case's series,
    as _latest_market_breadth / _market_breadth_recovery (:155-162) form them."""
    b = case["breadth"]
    return float(b[-1]), float(b[-1] - b[-3]) if len(b) >= 3 else float("nan")


def digest(p: dict[str, np.ndarray]) -> str:
    m = hashlib.sha256()
    for k in sorted(p):
        m.update(k.encode())
        m.update(np.ascontiguousarray(p[k]).tobytes())
    m.update(",".join(NAMES).encode())
    return m.hexdigest()
