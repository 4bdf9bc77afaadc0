"""Shared inputs of tests/test_sweep_ref.py and tests/test_sweep_gpu.py (and of
tests/golden/make_golden_sweep.py): the fixture tests/golden/sweep_gates.npz
with its regenerated panel, the near-tie count that lets a test demand exact
codes of columns computed on the device, and seeded gate columns with planted
candidates for the kernel's two mappings."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import sweep_panel_gen as pg   # noqa: E402
import sweep_ref as ref        # noqa: E402

TILE, ROW_CHUNK, SWITCH = 256, 64, 64   # bq_sweep_select: candles per wide tile, rows per chunk, the narrow width


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "sweep_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.sweep_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "sweep_panel_gen drifted from the recorded inputs"
    return p


def fixture_columns():
    """(cols, score_cross) of the fixture: the real compute_pump_score's values."""
    fx = fixture()
    return {k: fx["values"][:, :, i] for i, k in enumerate(ref.COLUMNS)}, fx["score_cross"]


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def near_tie_mask(cols, score_cross=None, *, first_t=None, lens=None, rel=1e-6, tiny=1e-12, **thresholds):
    """bool [S, T]: the cells whose frame is long enough and whose 13 values
    are finite, with a compare of the gate on a near-tie: two operands within
    `rel` relative of each other (both exactly 0 is no tie: the zeros of a
    clipped momentum are exact), or an operand compared with 0 that is within
    `tiny` of it without being 0. The compares: momentum_atr against its two
    bounds, close / prior_high, close_location / its bound, relative_volume /
    volume_threshold, close / ema20, pump_score / score_threshold at u and at
    u - 1 (score_cross' operands), and trend_score, relative_strength,
    btc_momentum_3, btc_trend_score, score_threshold against 0."""
    par = {**ref.DEFAULTS, **thresholds}
    x = {k: np.asarray(cols[k], np.float64) for k in ref.COLUMNS}
    S, T = x["close"].shape
    status, _ = ref.gate(cols, np.ones((S, T), bool), None, first_t, lens, **thresholds)
    at = (status != ref.NO_FRAME) & (status != ref.SHORT_FRAME) & (status != ref.NOT_FINITE)

    def close_to(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
        m = np.maximum(np.abs(a), np.abs(b))
        return (m > 0) & (np.abs(a - b) <= rel * m)

    n = np.zeros((S, T), bool)
    with np.errstate(all="ignore"):
        for a, b in ((x["momentum_atr"], par["min_momentum_atr"]), (x["momentum_atr"], par["max_momentum_atr"]),
                     (x["close"], x["prior_high"]), (x["close_location"], par["min_close_location"]),
                     (x["relative_volume"], x["volume_threshold"]), (x["close"], x["ema20"]),
                     (x["pump_score"], x["score_threshold"])):
            n |= close_to(a, b)
        prev = np.zeros((S, T), bool)
        prev[:, 1:] = close_to(x["pump_score"], x["score_threshold"])[:, :-1]
        n |= prev
        for k in ("trend_score", "relative_strength", "btc_momentum_3", "btc_trend_score", "score_threshold"):
            n |= (x[k] != 0) & (np.abs(x[k]) <= tiny)
    return n & at


def near_ties(*args, **kw) -> int:
    """How many cells near_tie_mask flags."""
    return int(near_tie_mask(*args, **kw).sum())


def planted_columns(S: int, T: int, seed: int, density: float = 0.06):
    """Seeded gate columns [S, T]: every cell starts as a passing candidate
    with a score in [1, 40); all but `density` of the cells are then spoiled at
    one random check (a NaN or inf among the required values, no cross, each
    compare on its failing side, a non-positive threshold) and sometimes at a
    later one too. Returns (cols, score_cross, route_ok)."""
    g = np.random.default_rng(seed)
    thr = g.uniform(0.05, 2.0, (S, T))
    c = dict(pump_score=thr * g.uniform(1.0, 40.0, (S, T)), score_threshold=thr,
             momentum_atr=g.uniform(0.8, 2.9, (S, T)), close=g.uniform(10.0, 11.0, (S, T)),
             prior_high=g.uniform(8.0, 9.9, (S, T)), close_location=g.uniform(0.71, 1.0, (S, T)),
             relative_volume=g.uniform(2.0, 5.0, (S, T)), volume_threshold=g.uniform(1.0, 1.9, (S, T)),
             trend_score=g.uniform(0.001, 0.05, (S, T)), ema20=g.uniform(9.0, 9.9, (S, T)),
             relative_strength=g.uniform(0.001, 0.05, (S, T)), btc_momentum_3=g.uniform(0.0005, 0.01, (S, T)),
             btc_trend_score=g.uniform(0.001, 0.03, (S, T)))
    cross = np.ones((S, T), bool)
    spoil = np.where(g.random((S, T)) < density, 0, g.integers(2, 14, (S, T)))
    again = np.where(g.random((S, T)) < 0.3, g.integers(2, 14, (S, T)), 0)
    for kind in (spoil, again):
        k = kind == ref.NOT_FINITE
        which = g.integers(0, len(ref.COLUMNS), (S, T))
        bad = g.choice([np.nan, np.inf, -np.inf], (S, T))
        for i, name in enumerate(ref.COLUMNS):
            c[name] = np.where(k & (which == i), bad, c[name])
        cross &= kind != ref.NO_CROSS
        c["momentum_atr"] = np.where(kind == ref.MOMENTUM_ATR, g.choice([0.5, 3.5], (S, T)), c["momentum_atr"])
        c["prior_high"] = np.where(kind == ref.NOT_ABOVE_PRIOR_HIGH, c["close"], c["prior_high"])
        c["close_location"] = np.where(kind == ref.CLOSE_LOCATION, 0.5, c["close_location"])
        c["volume_threshold"] = np.where(kind == ref.VOLUME, 6.0, c["volume_threshold"])
        c["trend_score"] = np.where(kind == ref.TREND, g.choice([0.0, -0.01], (S, T)), c["trend_score"])
        c["ema20"] = np.where(kind == ref.BELOW_EMA20, 11.5, c["ema20"])
        c["relative_strength"] = np.where(kind == ref.RELATIVE_STRENGTH, -0.002, c["relative_strength"])
        c["btc_momentum_3"] = np.where(kind == ref.BTC_MOMENTUM, 0.0, c["btc_momentum_3"])
        c["btc_trend_score"] = np.where(kind == ref.BTC_TREND, -0.001, c["btc_trend_score"])
        zero = kind == ref.THRESHOLD_NONPOSITIVE
        c["score_threshold"] = np.where(zero, 0.0, c["score_threshold"])
        c["pump_score"] = np.where(zero, g.uniform(0.0, 1.0, (S, T)), c["pump_score"])
    route_ok = g.random((S, T)) >= 0.2
    return c, cross, route_ok


def plant(c, cross, route_ok, s: int, t: int, score: float = 7.0):
    """Make cell (s, t) a candidate with rank_score `score` (inf: a finite
    pump_score whose quotient overflows)."""
    passing = dict(momentum_atr=1.5, close=10.5, prior_high=9.0, close_location=0.9, relative_volume=3.0,
                   volume_threshold=1.5, trend_score=0.01, ema20=9.5, relative_strength=0.01, btc_momentum_3=0.002,
                   btc_trend_score=0.01)
    for k, v in passing.items():
        c[k][s, t] = v
    if np.isinf(score):
        c["pump_score"][s, t], c["score_threshold"][s, t] = 1e300, 1e-300
    else:
        c["pump_score"][s, t], c["score_threshold"][s, t] = score * 0.5, 0.5
    cross[s, t] = True
    if route_ok is not None:
        route_ok[s, t] = True


def clear_column(c, cross, t: int):
    """No candidate in column t."""
    cross[:, t] = False
