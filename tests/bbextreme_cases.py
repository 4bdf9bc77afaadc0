"""Shared inputs of tests/test_bbextreme_ref.py and tests/test_bbextreme_gpu.py:
the fixture tests/golden/bbextreme_gates.npz with its regenerated panel, the
hand-built edge cases for the kernel's 64-candle step edges, and the
comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import bbextreme_panel_gen as pg   # noqa: E402
import bbextreme_ref as ref        # noqa: E402

WINDOWS = (2, 14)
BANDS = ("bb_upper", "bb_mid", "bb_lower")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "bbextreme_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.bbx_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "bbextreme_panel_gen drifted from the recorded inputs"
    return p


def recorded(window: int = 2) -> dict:
    """The recording at rsi_window `window` in replay()'s output layout."""
    fx = fixture()
    sfx = "" if window == WINDOWS[0] else f"_w{window}"
    return {k: fx[k + sfx] for k in ("status", "autotrade", "route") + ref.VALUES}


def ref_replay(p: dict, **kw):
    return ref.replay(p["close"], p["bb_upper"], p["bb_mid"], p["bb_lower"], **kw)


@functools.lru_cache(maxsize=4)
def fixture_replay(window: int, direct: bool = False):
    """The restatement on the fixture panel (computed once; do not modify)."""
    p = panel()
    return ref_replay(p, first_t=p["first_t"], lens=p["lens"], rsi_window=window,
                      rsi=ref.frame_rsi_direct if direct else ref.frame_rsi)


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


def edge_panel(S: int, T: int, seed: int, lookback: int = 30, window: int = 2) -> dict:
    """A walk dense in what the kernel can get wrong, every few candles: runs
    of falling and of rising candles at the band (emitted buys and sells),
    spikes of up to 2^60 and collapses, flat runs, and per row s (where they
    fit): a NaN close exactly `lookback` and `lookback - 1` candles before
    the newest candle (rows 0 / 1), an infinite close `window` and `window +
    1` candles before it (rows 2 / 3), a zero close (row 4), and a NaN and an
    infinite close on lanes 63 and 0 of a step. Bands: the close -+ a small
    offset that the runs cross, with cells of zero, negative and NaN span and
    of bb_mid <= 0 / NaN."""
    rng = np.random.default_rng(seed)
    k = np.arange(T)
    drift = np.where((k // 3) % 2 == 0, -0.006, 0.006)
    close = 10.0 ** rng.uniform(-1, 2, (S, 1)) * np.exp(np.cumsum(drift[None, :] + rng.normal(0.0, 0.004, (S, T)), axis=1))
    for s in range(S):
        for t in range(int(rng.integers(2, 9)), T, int(rng.integers(7, 13))):
            u = rng.random()
            if u < 0.35:
                close[s, t:] *= 2.0 ** rng.uniform(-30, 60)
            elif u < 0.6:
                close[s, t] *= 2.0 ** rng.uniform(-30, 60)
            elif u < 0.8:
                close[s, t:t + 3] = close[s, t - 1]
            if close[s, t] > 1e200 or close[s, t] < 1e-200:
                close[s, t:] *= close[s, 0] / close[s, t]
    prev = np.concatenate([close[:, :1], close[:, :-1]], axis=1)
    mid = (close + prev) / 2
    half = np.abs(close - prev) * rng.uniform(0.2, 0.9, (S, T)) + 1e-3 * np.abs(mid)
    up, lo = mid + half, mid - half
    kind = rng.random((S, T))
    up = np.where(kind < 0.03, lo, up)
    up, lo = np.where((kind >= 0.03) & (kind < 0.06), lo, up), np.where((kind >= 0.03) & (kind < 0.06), up, lo)
    up = np.where((kind >= 0.06) & (kind < 0.08), np.nan, up)
    mid = np.where((kind >= 0.08) & (kind < 0.1), 0.0, mid)
    mid = np.where((kind >= 0.1) & (kind < 0.12), np.nan, mid)
    mid = np.where((kind >= 0.12) & (kind < 0.14), -mid, mid)
    last = T - 1
    plant = {0: (last - lookback, np.nan), 1: (last - lookback + 1, np.nan), 2: (last - window, np.inf),
             3: (last - window - 1, -np.inf), 4: (last - 3, 0.0)}
    for s, (t, v) in plant.items():
        if s < S and 0 <= t < T:
            close[s, t] = v
    if S > 4 and T > 70:
        close[4, 63], close[4, 64] = np.nan, np.inf
    return dict(close=close, bb_upper=up, bb_mid=mid, bb_lower=lo)
