"""Shared inputs of tests/test_pricetracker_ref.py and
tests/test_pricetracker_gpu.py: the fixture tests/golden/pricetracker_gates.npz
with its regenerated panel, seeded panels for the kernel's 64-candle step
edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import pricetracker_panel_gen as pg   # noqa: E402
import pricetracker_ref as ref        # noqa: E402

STEP = pg.STEP_MS
WAVE = 64   # candles per step of price_tracker_kernel
PANELS = ("close", "rsi", "macd", "mfi")
RECORDED = {"local_score": "local_score", "trend_score": "trend_score", "followthrough": "followthrough",
            "adverse_risk": "adverse_risk", "supportiveness": "supportiveness", "adjusted_score": "adjusted_score"}


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "pricetracker_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.price_tracker_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "pricetracker_panel_gen drifted from the recorded inputs"
    return p


def same_bits(a, b) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_codes_equal(got, want, what=""):
    for name in ("status", "detail"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"


def assert_values_bits(got, want, what="", names=ref.VALUES):
    for name in names:
        bad = np.argwhere(~same_bits(got[name], want[name]))
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(got[name][tuple(i)], want[name][tuple(i)]) for i in bad[:5]]}"


def assert_values_close(got, want, what="", trend_rtol=1e-9, atol=1e-9):
    """trend_score at trend_rtol relative, the score fields at atol absolute;
    NaN exactly where the reference has NaN."""
    for name in ref.VALUES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert (np.isnan(g) == np.isnan(w)).all(), f"{what}: {name}: NaN pattern differs"
        m = ~np.isnan(w)
        err = np.abs(g[m] - w[m])
        bound = trend_rtol * np.abs(w[m]) if name == "trend_score" else atol
        assert (err <= bound).all(), f"{what}: {name}: max error {err.max()} (bound {np.max(bound)})"


def assert_state_equal(got, want, what=""):
    gh, gl = (np.asarray(x) for x in got)
    wh, wl = (np.asarray(x) for x in want)
    assert (gh.astype(bool) == wh.astype(bool)).all(), f"{what}: has differs"
    m = wh.astype(bool)
    assert (gl[m] == wl[m]).all(), f"{what}: last_close_time differs"


def recorded(fx=None) -> dict:
    """The recording in replay()'s output layout."""
    fx = fx or fixture()
    out = {k: fx[v] for k, v in RECORDED.items()}
    out.update(status=fx["status"], detail=fx["detail"])
    return out


def fixture_kwargs(with_trend: bool) -> dict:
    """replay()'s keyword inputs on the fixture panel (numpy)."""
    fx, p = fixture(), panel()
    kw = dict(symbol_rs=p["symbol_rs"], ctx=p["ctx"], ctx_ok=p["ctx_ok"], high=p["high"], low=p["low"],
              volume=p["volume"], first_t=p["first_t"], lens=p["lens"])
    if with_trend:
        kw["trend_score"] = fx["trend_score"]
    return kw


def seeded_panel(S: int, T: int, seed: int, *, setup_rate=0.5, nan_at=(), gap_rows=(), per_candle_ctx=True) -> dict:
    """A random panel dense in oversold cells: cooldown windows overlap every
    step edge. nan_at: (row, candle, column) cells set to NaN; gap_rows: rows
    whose close_time jumps by 9 bars at T // 2. The closes drift (0.6 % a
    candle against 0.2 % noise), so ema9 - ema21 stays near 3.6 % of the
    price: trend_score is a difference, and at a zero crossing its relative
    error is unbounded for any summation order — pandas' own rounding,
    3 u (1 / alpha9 + 1 / alpha21) ~ 5e-15 absolute, is already above 1e-9
    relative once |trend_score| < 5e-6. Away from a crossing the 1e-9
    relative bar is meaningful and is what the tests hold."""
    rng = np.random.default_rng(seed)
    close = 10.0 ** rng.uniform(-1, 2, (S, 1)) * np.exp(np.cumsum(rng.normal(0.006, 0.002, (S, T)), axis=1))
    p = dict(close=close, high=close * 1.002, low=close * 0.998, volume=rng.lognormal(3, 1, (S, T)),
             rsi=np.where(rng.random((S, T)) < setup_rate, rng.uniform(10, 29, (S, T)), rng.uniform(31, 60, (S, T))),
             macd=-np.abs(rng.normal(0.004, 0.004, (S, T))) - 1e-4, mfi=rng.uniform(3, 19, (S, T)))
    ct = np.tile(pg.T0_MS + (np.arange(T, dtype=np.int64) + 1) * STEP - 1, (S, 1))
    for s in gap_rows:
        ct[s, T // 2:] += 9 * STEP
    Tc = T if per_candle_ctx else 1
    ctx = np.stack([rng.uniform(0.3, 0.95, Tc), rng.uniform(-0.6, 0.6, Tc), rng.uniform(-0.5, 0.7, Tc),
                    rng.uniform(0.05, 0.7, Tc)])
    ctx[0][rng.random(Tc) < 0.05] = 0.0
    p.update(close_time=ct, ctx=ctx, ctx_ok=rng.random(Tc) > 0.08, symbol_rs=rng.normal(0.0, 0.03, (S, T)))
    for s, t, col in nan_at:
        if s < S and t < T:
            p[col][s, t] = np.nan
    return p


def replay_kwargs(p: dict, **extra) -> dict:
    kw = dict(symbol_rs=p["symbol_rs"], ctx=p["ctx"], ctx_ok=p["ctx_ok"], high=p["high"], low=p["low"],
              volume=p["volume"])
    kw.update(extra)
    return kw


def ref_replay(p: dict, **kw):
    return ref.replay(*(p[k] for k in PANELS), p["close_time"], **kw)
