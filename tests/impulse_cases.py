"""Shared inputs of tests/test_impulse_ref.py and tests/test_impulse_gpu.py:
the fixture tests/golden/impulse_gates.npz with its regenerated panel, the
runs it records, seeded panels with injected impulses, and a bit-for-bit
comparison."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import impulse_panel_gen as pg   # noqa: E402
import impulse_ref as ref        # noqa: E402

STEP = 900_000
T0 = 1_760_400_000_000


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "impulse_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.impulse_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "impulse_panel_gen drifted from the recorded inputs"
    return p


def runs():
    """name -> (symbols, benchmark key, thresholds): the recorded runs of the
    fixture (make_golden_impulse.py)."""
    fx = fixture()
    out = {"a_A": (range(pg.S), "a", {}), "a_B": (range(16), "b", {}), "inf_A": (range(pg.S), "a", dict(ref.WIDE_OPEN))}
    for i, m in enumerate(fx["min_impulse_grid"]):
        out[f"g{i}_A"] = (range(pg.S), "a", {**ref.WIDE_OPEN, "min_impulse": float(m)})
        if f"g{i}_B_status" in fx:
            out[f"g{i}_B"] = (range(16), "b", {**ref.WIDE_OPEN, "min_impulse": float(m)})
    return out


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_gate_equal(values, status, want_values, want_status, what=""):
    """status exact, values bit-equal, NaN exactly where status != 0."""
    status, want_status = np.asarray(status), np.asarray(want_status)
    bad = np.argwhere(status != want_status)
    assert len(bad) == 0, f"{what}: status differs at {bad[:5].tolist()}: " \
                          f"{[(int(status[tuple(i)]), int(want_status[tuple(i)])) for i in bad[:5]]}"
    for k, want in want_values.items():
        got = np.asarray(values[k])
        eq = same_bits(got, want)
        assert eq.all(), f"{what}: {k} differs at {np.argwhere(~eq)[:5].tolist()}"
        assert (np.isnan(got) == (status != 0)).all(), f"{what}: {k} NaN pattern is not status != 0"


def injected_panel(S: int, T: int, seed: int, tile: int = 1024, nan_rate: float = 0.002):
    """Seeded walks [S, T] with an impulse (trigger / confirmation pair) about
    every 23 candles and one around every multiple of `tile`, so that the pairs and
    their t - 6 anchors straddle tile boundaries; a few NaN / zero closes,
    flat confirmations and NaN ATRs. Returns a dict of arrays and a regular
    benchmark frame on the panel's grid."""
    g = np.random.default_rng(seed)
    r = g.normal(0.0, 0.005, (S, T))
    for s in range(S):
        spots = set(range(25, T - 1, 23))
        for b in range(tile, T + tile, tile):   # one trigger per row within [b - 3, b + 6] of each tile boundary
            tr = b + int(g.integers(-3, 7))
            spots -= set(range(tr - 6, tr + 8))
            if 7 <= tr < T - 1:
                spots.add(tr)
        for tr in sorted(spots):
            if g.random() < 0.6 or tr % tile < 7 or tr % tile >= tile - 3:
                r[s, max(tr - 5, 0):tr] = g.normal(0.0, 0.0008, tr - max(tr - 5, 0))
                r[s, tr] = np.log(1.0 + g.uniform(0.03, 0.2))
                r[s, tr + 1] = g.uniform(-0.004, 0.008)
    c = 10.0 ** g.uniform(-2, 3, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 0.002, (S, T)))
    l = np.minimum(o, c) * (1.0 - g.uniform(0.0, 0.002, (S, T)))
    atr = c * g.uniform(0.01, 0.07, (S, T))
    for arr, val in ((c, np.nan), (c, 0.0), (atr, np.nan), (o, -1.0)):
        arr[g.random((S, T)) < nan_rate] = val
    flat = g.random((S, T)) < nan_rate
    h[flat] = l[flat]
    ts = np.broadcast_to(T0 + STEP * np.arange(T, dtype=np.int64), (S, T)).copy()
    b_ts = T0 + STEP * np.arange(T, dtype=np.int64)
    b_close = 60000.0 * np.exp(np.cumsum(g.normal(0.0, 0.001, T)))
    return dict(open=o, high=h, low=l, close=c, atr=atr, open_time=ts), b_ts, b_close
