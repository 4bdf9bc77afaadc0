"""Shared inputs of tests/test_dip_ref.py and tests/test_dip_gpu.py: the fixture
tests/golden/dip_gates.npz with its regenerated panel, seeded panels for the
kernel's 64-candle step edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import dip_panel_gen as pg   # noqa: E402
import dip_ref as ref        # noqa: E402

STEP = pg.STEP_MS
POINTWISE = ("reference_price", "change_6h")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "dip_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.dip_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "dip_panel_gen drifted from the recorded inputs"
    return p


def recorded(fx=None) -> dict:
    """The recording in replay()'s output layout."""
    fx = fx or fixture()
    return {k: fx[k] for k in ("status",) + ref.VALUES}


def fixture_kwargs(with_ema: bool) -> dict:
    """replay()'s keyword inputs on the fixture panel (numpy)."""
    fx, p = fixture(), panel()
    kw = dict(market_regime=p["market_regime"], micro_regime=pg.micro_code(p), first_t=p["first_t"], lens=p["lens"])
    if with_ema:
        kw["ema20"] = fx["ema20"]
    return kw


def same_bits(a, b) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_codes_equal(got, want, what=""):
    g, w = np.asarray(got["status"]), np.asarray(want["status"])
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: status differs at {bad[:5].tolist()}: " \
                          f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"


def assert_values_bits(got, want, what="", names=ref.VALUES):
    for name in names:
        bad = np.argwhere(~same_bits(got[name], want[name]))
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(got[name][tuple(i)], want[name][tuple(i)]) for i in bad[:5]]}"


def assert_ema_close(got, want, what="", rtol=1e-9):
    """ema20 at rtol relative (DESIGN §3's bar for in-pass EMAs); NaN exactly
    where the reference has NaN."""
    g, w = np.asarray(got["ema20"]), np.asarray(want["ema20"])
    assert (np.isnan(g) == np.isnan(w)).all(), f"{what}: ema20: NaN pattern differs"
    m = ~np.isnan(w)
    err = np.abs(g[m] - w[m])
    assert (err <= rtol * np.abs(w[m])).all(), f"{what}: ema20: max relative error {(err / np.abs(w[m])).max()}"


def seeded_panel(S: int, T: int, seed: int, *, nan_at=(), gap_rows=(), dense_rows=(), specials=True) -> dict:
    """A random panel dense in dips that reclaim: a 32-candle pattern (a 6 %
    drop over three candles, a flat floor of 17, a recovery of 3.2 % over four
    candles and of 2.8 % over the next four, four flat candles) under 0.4 %
    noise: the candles of the first recovery are 2.8-4.4 % below the close 24
    candles before them and above the floor's EMA, so every code from the
    search on occurs in every step. Every close_time is past START_TIME but
    for row 0's first 30 candles.
    gap_rows: rows whose close_time jumps by 9 bars at T // 2 and by 30 bars
    (more than six hours) at 3 T // 4; dense_rows: rows of 5-minute candles
    (the reference is 72 candles back: two steps); nan_at: (row, candle)
    closes set to NaN; specials: a zero close (row 1, candle 40) and infinite
    closes 24 candles apart (row 2, candles 50 and 74) where they fit."""
    rng = np.random.default_rng(seed)
    k = np.arange(T)
    j = (k + 5) % 32
    saw = np.select([j < 3, j < 20, j < 24, j < 28], [-0.02, 0.0, 0.008, 0.007], 0.0)
    close = 10.0 ** rng.uniform(-1, 2, (S, 1)) * np.exp(np.cumsum(saw[None, :] * rng.uniform(0.8, 1.2, (S, 1))
                                                                  + rng.normal(0.0, 0.004, (S, T)), axis=1))
    ct = np.tile(pg.START_MS + (k.astype(np.int64) + 1) * STEP - 1, (S, 1))
    ct[0] -= 30 * STEP
    for s in gap_rows:
        if s < S:
            ct[s, T // 2:] += 9 * STEP
            ct[s, 3 * T // 4:] += 30 * STEP
    for s in dense_rows:
        if s < S:
            ct[s] = pg.START_MS + 1_000 + k.astype(np.int64) * pg.DENSE_STEP_MS
    p = dict(close=close, close_time=ct,
             market_regime=rng.choice([-1, 0, 1, 2, 3, 4], T, p=[0.1, 0.05, 0.05, 0.5, 0.1, 0.2]).astype(np.int8),
             micro_regime=rng.choice([-1, 0, 1, 2, 3, 4], (S, T), p=[0.1, 0.05, 0.05, 0.5, 0.1, 0.2]).astype(np.int8))
    for s, t in nan_at:
        if s < S and t < T:
            close[s, t] = np.nan
    if specials:
        if S > 1 and T > 40:
            close[1, 40] = 0.0
        if S > 2 and T > 74:
            close[2, 50] = close[2, 74] = np.inf
    return p


def ref_replay(p: dict, **kw):
    kw.setdefault("market_regime", p["market_regime"])
    kw.setdefault("micro_regime", p["micro_regime"])
    return ref.replay(p["close"], p["close_time"], **kw)
