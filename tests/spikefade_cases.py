"""Shared inputs of tests/test_spikefade_ref.py and tests/test_spikefade_gpu.py:
the fixture tests/golden/spikefade_gates.npz with its regenerated panel,
synthetic panels whose pending spikes straddle the kernel's 64-candle steps,
and the comparisons (everything exact)."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import spikefade_panel_gen as pg   # noqa: E402
import spikefade_ref as ref        # noqa: E402

STEP = 900_000
T0 = 1_760_400_000_000
WAVE = 64   # candles per step of spike_fade_kernel
COLS = ("open", "high", "close")
SPIKE_FIELDS = ("label", "price_break_flag", "cumulative_price_break_flag", "accel_spike_flag", "close_open_ratio",
                "upward")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "spikefade_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.fade_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "spikefade_panel_gen drifted from the recorded inputs"
    return p


def fixture_params():
    fx = fixture()
    return dict(window_bars=int(fx["window_bars"]), ext_factor=float(fx["ext_factor"]))


def fixture_inputs():
    """The replay's inputs on the fixture panel (numpy): the panel's prices
    and times, the recorded per-frame source_ok and market gates."""
    fx, p = fixture(), panel()
    return {**{k: p[k] for k in COLS + ("open_time",)}, "source_ok": fx["source_ok"], "src_market": fx["src_market"],
            "fail_market": fx["fail_market"]}


def same_bits(a, b) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_replay_equal(got, want, what="", cols=slice(None)):
    """(event, detail, bars): all exact."""
    for name, g, w in zip(("event", "detail", "bars"), got[:3], want[:3]):
        g, w = np.asarray(g)[:, cols], np.asarray(w)[:, cols]
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"


def assert_state_equal(got, want, what=""):
    """(active, open_time, high, close): the last three compared where active."""
    ga, wa = np.asarray(got[0]).astype(bool), np.asarray(want[0]).astype(bool)
    assert (ga == wa).all(), f"{what}: active differs at rows {np.argwhere(ga != wa)[:5].ravel().tolist()}"
    assert (np.asarray(got[1])[wa] == np.asarray(want[1])[wa]).all(), f"{what}: open_time differs"
    for i, name in ((2, "high"), (3, "close")):
        assert same_bits(np.asarray(got[i])[wa], np.asarray(want[i])[wa]).all(), f"{what}: {name} differs"


def recorded_state(t_at: np.ndarray, rows=None):
    """The fixture's strategy_states entry of the rows after candle t_at[s]
    (idle where t_at[s] is before the row's first candle)."""
    fx = fixture()
    rows = np.arange(pg.S) if rows is None else np.asarray(rows)
    t_at = np.asarray(t_at)
    t = np.maximum(t_at, 0)
    active = np.where(t_at >= 0, fx["st_active"][rows, t], False)
    return (active.astype(np.uint8), np.where(active, fx["st_open_time"][rows, t], 0).astype(np.int64),
            np.where(active, fx["st_high"][rows, t], np.nan), np.where(active, fx["st_close"][rows, t], np.nan))


def idle_state(S: int):
    return np.zeros(S, np.uint8), np.zeros(S, np.int64), np.full(S, np.nan), np.full(S, np.nan)


def edge_panel(S: int, T: int, seed: int, window: int = 8):
    """S rows x T candles of synthetic prices and masks around the kernel's
    step edges. Prices: a small walk whose highs revisit recent highs often,
    with red and green candles mixed, so that failed new highs, extensions
    (7 % wicks) and quiet windows all occur. By row (mod 6):
      0  sources at lane 63 of every step, the failure gate open at lane 0 of
         the next one and a failed new high made there;
      1  sources `window` candles before each step edge: the candidate gate
         opens at bars == window on odd steps (the failing candle is made
         there), never on even ones (the expiry at bars == window + 1 lies
         across the edge);
      2  dense sources and open gates: three or more set / resolve cycles
         inside a step;
      3  sparse sources, the source market gate shut half of the time;
      4  3 % of the highs missing, and runs of missing highs;
      5  dense sources, every high of some windows missing.
    Returns the dict of inputs (masks bool [S, T])."""
    g = np.random.default_rng(seed)
    r = g.normal(0.0, 0.004, (S, T))
    c = 10.0 ** g.uniform(-2, 3, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    wick = np.where(g.random((S, T)) < 0.04, 0.07, np.where(g.random((S, T)) < 0.5, 0.012, 0.001))
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 1.0, (S, T)) * wick)
    lane = np.arange(T) % WAVE
    step = np.arange(T) // WAVE
    kind = np.arange(S) % 6
    dens = np.array([0.0, 0.0, 0.35, 0.03, 0.08, 0.3])[kind][:, None]
    source = g.random((S, T)) < dens
    src_m = g.random((S, T)) < np.where(kind == 3, 0.5, 0.9)[:, None]
    fail_m = g.random((S, T)) < np.array([0.2, 0.0, 0.7, 0.4, 0.5, 0.5])[kind][:, None]
    for s in range(S):
        if kind[s] == 0:
            source[s], src_m[s] = lane == WAVE - 1, True
            fail_m[s] = lane == 0
        elif kind[s] == 1:
            source[s], src_m[s] = lane == (WAVE - window) % WAVE, True
            fail_m[s] = (lane == 0) & (step % 2 == 1) if window < WAVE else False
        if kind[s] in (0, 1):   # the candle at lane 0 fails the spike `window` (or 1) candles before it
            back = 1 if kind[s] == 0 else window
            h[s, 1:] = np.maximum(o[s, 1:], c[s, 1:]) * (1.0 + g.uniform(0.0, 0.0005, T - 1))
            for t in range(back, T):
                if lane[t] == 0:
                    h[s, t - back] = max(np.nanmax(h[s, t - back:t + 1]), h[s, t - back]) * 1.0001
                    c[s, t] = min(c[s, t - back], o[s, t]) * 0.999
                    if t + 1 < T:
                        o[s, t + 1] = c[s, t]
                    h[s, t] = h[s, t - back] * 1.0002
        if kind[s] == 4:
            h[s, g.random(T) < 0.03] = np.nan
            for b in range(17, T - 6, 41):
                h[s, b:b + 5] = np.nan
        if kind[s] == 5:
            for b in range(5, T - 12, 29):
                h[s, b:b + 12] = np.nan
    ts = T0 + STEP * np.arange(T, dtype=np.int64)[None, :] + np.zeros((S, 1), np.int64)
    return dict(open=o, high=h, close=c, open_time=ts, source_ok=source, src_market=src_m, fail_market=fail_m)


def replay_ref(p, **kw):
    return ref.spike_fade_replay(*(p[k] for k in COLS), p["open_time"], p["source_ok"], p.get("src_market"),
                                 p.get("fail_market"), **kw)
