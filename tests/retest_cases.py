"""Shared inputs of tests/test_retest_ref.py and tests/test_retest_gpu.py: the
fixture tests/golden/retest_gates.npz with its regenerated panel, seeded
panels whose watches straddle the kernel's 64-candle steps, and the
comparisons (everything exact)."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import retest_panel_gen as pg   # noqa: E402
import retest_ref as ref        # noqa: E402

STEP = 900_000
T0 = 1_760_400_000_000
WAVE = 64   # candles per step of retest_kernel
COLS = ("open", "high", "low", "close")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "retest_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.retest_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "retest_panel_gen drifted from the recorded inputs"
    return p


def fixture_params():
    fx = fixture()
    return dict(watch_ms=int(fx["watch_ms"]), min_history=int(fx["min_history"]),
                breakout_lookback=int(fx["breakout_lookback"]), support_factor=float(fx["support_factor"]),
                pullback_factor=float(fx["pullback_factor"]))


def same_bits(a, b) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_replay_equal(got, want, what="", cols=slice(None)):
    """(event, detail, level): events and details exact, levels bit for bit."""
    for name, g, w in zip(("event", "detail"), got[:2], want[:2]):
        g, w = np.asarray(g)[:, cols], np.asarray(w)[:, cols]
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"
    eq = same_bits(np.asarray(got[2])[:, cols], np.asarray(want[2])[:, cols])
    assert eq.all(), f"{what}: level differs at {np.argwhere(~eq)[:5].tolist()}"


def assert_state_equal(got, want, what=""):
    """(active, started, level): started and level compared where active."""
    ga, wa = np.asarray(got[0]).astype(bool), np.asarray(want[0]).astype(bool)
    assert (ga == wa).all(), f"{what}: active differs at rows {np.argwhere(ga != wa)[:5].ravel().tolist()}"
    assert (np.asarray(got[1])[wa] == np.asarray(want[1])[wa]).all(), f"{what}: started differs"
    assert same_bits(np.asarray(got[2])[wa], np.asarray(want[2])[wa]).all(), f"{what}: level differs"


def recorded_state(t_at: np.ndarray):
    """The fixture's strategy_states entry of every row after candle t_at[s]
    (idle where t_at[s] is before the row's first candle)."""
    fx, rows = fixture(), np.arange(pg.S)
    t = np.maximum(t_at, 0)
    active = np.where(t_at >= 0, fx["st_active"][rows, t], False)
    return (active.astype(np.uint8), np.where(active, fx["st_started"][rows, t], 0).astype(np.int64),
            np.where(active, fx["st_level"][rows, t], np.nan))


# parameters of the step-edge panels: a short history so that T = 63 holds watches, and a watch of 20 candles
EDGE_PARAMS = dict(min_history=12, watch_ms=20 * STEP, breakout_lookback=8)
EDGE_S = 6


def edge_panel(T: int, seed: int):
    """EDGE_S rows x T candles. Rows 0-1: leaders at lanes 0 and 63 of every
    step (the level's window reaches back across the step), sparse green
    candles (watches cross steps, expire or resolve in a later one); rows
    2-3: dense leaders and green candles; row 4: time gaps; row 5: 3 % NaN
    highs / lows. Returns the dict of inputs (leader / risk_ok bool)."""
    g = np.random.default_rng(seed)
    S = EDGE_S
    r = g.normal(0.0, 0.004, (S, T))
    c = 10.0 ** g.uniform(-2, 3, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    wick = np.where(np.arange(S)[:, None] < 2, 0.012, 0.001)   # rows 0-1: long upper wicks, few reclaims
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 1.0, (S, T)) * wick)
    l = np.minimum(o, c) * (1.0 - g.uniform(0.0, 0.004, (S, T)))
    ema = c * (1.0 + g.normal(0.0, 0.004, (S, T)))
    lane = np.arange(T) % WAVE
    leader = g.random((S, T)) < np.array([0.0, 0.01, 0.3, 0.1, 0.06, 0.06])[:, None]
    leader[:2] |= (lane == 0) | (lane == WAVE - 1)
    risk = g.random((S, T)) < 0.6
    dt = np.full((S, T), STEP, np.int64)
    dt[4] += STEP * (g.random(T) < 0.1) * g.integers(1, 30, T)
    ts = T0 + np.cumsum(dt, axis=1) - STEP
    for a in (h, l):
        a[5, g.random(T) < 0.03] = np.nan
    return dict(open=o, high=h, low=l, close=c, ema=ema, open_time=ts, leader=leader, risk_ok=risk)
