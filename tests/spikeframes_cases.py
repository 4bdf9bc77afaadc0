"""Shared inputs of tests/test_spikeframes_ref.py, test_spikeframes_args.py and
test_spikeframes_gpu.py: the fixture tests/golden/spikeframes.npz with its
regenerated panel, the second yardstick (spikefade_gates.npz's recorded
last_spike fields), the restatement's results (computed once, shared) and
synthetic panels for the kernel's edges."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import spikefade_panel_gen as fade_pg     # noqa: E402
import spikeframes_panel_gen as pg        # noqa: E402
import spikeframes_ref as ref             # noqa: E402

OHLCV = ("open", "high", "low", "close", "volume", "quote_asset_volume")
FADE_FIELDS = ("label", "price_break_flag", "cumulative_price_break_flag", "accel_spike_flag", "upward")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "spikeframes.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.frames_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "spikeframes_panel_gen drifted from the recorded inputs"
    return p


@functools.lru_cache(maxsize=1)
def fade_fixture():
    z = np.load(GOLDEN / "spikefade_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def fade_panel():
    p = fade_pg.fade_panel()
    assert fade_pg.digest(p) == str(fade_fixture()["digest"])
    return p


def in_frame(p) -> np.ndarray:
    cols = np.arange(p["close"].shape[1])
    return (cols >= p["first_t"][:, None]) & (cols < p["lens"][:, None])


@functools.lru_cache(maxsize=4)
def ref_fixture(back_walk: bool = False):
    """The restatement on the fixture panel, and the back-walk lengths it took."""
    p, walks = panel(), []
    return ref.frames(p["open"], p["close"], p["volume"], first_t=p["first_t"], lens=p["lens"], back_walk=back_walk,
                      walks=walks), np.array(walks)


@functools.lru_cache(maxsize=1)
def ref_fade():
    p = fade_panel()
    return ref.frames(p["open"], p["close"], p["volume"], first_t=p["first_t"], lens=p["lens"], back_walk=True)


def same_bits(a, b) -> np.ndarray:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_bools_equal(got, want, mask, what, keys=ref.BOOL_KEYS):
    for k in keys:
        g, w = np.asarray(got[k]).astype(bool), np.asarray(want[k]).astype(bool)
        bad = np.argwhere((g != w) & mask)
        assert len(bad) == 0, f"{what}: {k} differs at {bad[:6].tolist()} ({len(bad)} cells)"


def assert_fill(got, mask, what):
    """Outside the formed candles: False / NaN (close_open_ratio is formed wherever the candle is)."""
    for k in ref.BOOL_KEYS:
        if k in got:
            assert not np.asarray(got[k]).astype(bool)[~mask].any(), f"{what}: {k} outside the frame"
    for k in ("volume_cluster_min_ratio", "price_break_base_threshold"):
        if k in got:
            assert np.isnan(np.asarray(got[k])[~mask]).all(), f"{what}: {k} outside the frame"


def synth_panel(S: int, T: int, seed: int, kind: str = "mixed") -> dict[str, np.ndarray]:
    """S x T candles for the kernel's edges. kind: 'mixed' (by row mod 4: a
    quiet walk with spikes, a dense-spike row, a noisy row, a row with 6 % of
    the candles missing), 'nan' (every close and volume missing), 'equal'
    (every candle the same: ties in the ranking), 'dense5' (a qualifying
    bullish spike every 5 bars from candle 20 on: the back-walk reaches the
    frame's first row across several 64-candle blocks)."""
    g = np.random.default_rng(seed)
    r = g.normal(0.0, 0.002, (S, T))
    vol = g.lognormal(3.0, 0.3, (S, T))
    for s in range(S):
        k = s % 4 if kind == "mixed" else 0
        if kind in ("nan", "equal"):
            continue
        if k == 2:
            r[s] = g.normal(0.0, 0.03, T)
        t = 14 + int(g.integers(0, 5)) if kind == "mixed" else 20
        while t < T:
            r[s, t] = g.uniform(0.02, 0.05) * (-1.0 if kind == "mixed" and g.random() < 0.25 else 1.0)
            vol[s, t] *= g.uniform(2.5, 5.0)
            t += 5 if kind == "dense5" else int(g.integers(4, 7)) if k == 1 else int(g.integers(6, 25))
    c = 10.0 ** g.uniform(-1, 3, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    if kind == "equal":
        c = np.full((S, T), 25.0)
        vol = np.full((S, T), 40.0)
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * 1.001
    l = np.minimum(o, c) * 0.999
    qv = vol * c
    if kind == "nan":
        c, vol, qv = (np.full((S, T), np.nan) for _ in range(3))
    if kind == "mixed":
        for s in range(3, S, 4):
            hole = g.random(T) < 0.06
            c[s], vol[s], qv[s] = (np.where(hole, np.nan, x[s]) for x in (c, vol, qv))
    return dict(open=o, high=h, low=l, close=c, volume=vol, quote_asset_volume=qv)
