"""Shared inputs of tests/test_topgainer_ref.py and tests/test_topgainer_gpu.py
(and of tests/golden/make_golden_topgainer.py): the fixture
tests/golden/topgainer_gates.npz with its regenerated panel, the runs it
records, seeded panels with injected breakouts around tile boundaries, the
near-tie count that lets a test demand exact codes, and the comparison."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import topgainer_panel_gen as pg   # noqa: E402
import topgainer_ref as ref        # noqa: E402
from util import assert_close      # noqa: E402

INPUTS = ("open", "high", "low", "close", "volume")
# run name -> (quote_volume and ATR columns given, value columns recorded)
RUNS = {"qa": (True, ref.TGE_KEYS), "plain": (False, ("quote_volume", "quote_volume_ratio", "atr"))}


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "topgainer_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.topgainer_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "topgainer_panel_gen drifted from the recorded inputs"
    return p


def run_args(p, name, rows=slice(None)):
    """(positional arrays, keywords) of a recorded run: open .. volume, then
    quote_volume / atr or None."""
    with_qa, _ = RUNS[name]
    args = [p[k][rows] for k in INPUTS] + [p["quote_volume"][rows] if with_qa else None,
                                           p["atr"][rows] if with_qa else None]
    return args, dict(risk_ok=p["risk_ok"][rows], first_t=p["first_t"][rows])


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: both NaN, or the same fp64 bits."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


def assert_entry_equal(got, want, what="", keys=None):
    """status / entry exact; point-wise values bit for bit; ema20 / ema50, the
    two volume ratios and score within tests/util's 1e-9 (NaN patterns equal);
    stop_loss_pct bit for bit."""
    for k in ("status", "entry"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {k} differs at {bad[:5].tolist()}: " \
                              f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"
    for k in (keys if keys is not None else want["values"]):
        g, w = np.asarray(got["values"][k]), np.asarray(want["values"][k])
        if k in ref.APPROX_KEYS:
            # the scale of a ratio's error is the ratio itself; the ewm columns' is the price
            assert_close(g, w, f"{what}: {k}", scale=np.abs(np.where(np.isnan(w), 0.0, w)))
        else:
            eq = same_bits(g, w)
            assert eq.all(), f"{what}: {k} differs at {np.argwhere(~eq)[:5].tolist()}"
    assert_close(got["score"], want["score"], f"{what}: score", scale=1.0)
    eq = same_bits(got["stop_loss_pct"], want["stop_loss_pct"])
    assert eq.all(), f"{what}: stop_loss_pct differs at {np.argwhere(~eq)[:5].tolist()}"


def near_tie_mask(o, h, l, c, v, qv=None, atr=None, *, first_t=None, lens=None, at=None, rel=1e-6, **thresholds):
    """bool [S, T]: the candles with a gate decision on a near-tie, from the
    restatement's raw values at the candles `at` (bool [S, T]; None: all)
    whose features are ready: |close - ema20|, |close - ema50| and
    |volume_ratio - threshold| within `rel` relative (the values compared at
    1e-9), and every point-wise operand equal to its threshold (the bit-exact
    values), the two confirmation compares included."""
    par = {**ref.DEFAULTS, **thresholds}
    r = ref.top_gainer_entry(o, h, l, c, v, qv, atr, first_t=first_t, lens=lens, raw=True, **thresholds)
    x = r["values"]
    ready = (r["entry"] == 0) | ((r["entry"] >= 4) & (r["entry"] <= 14))
    if at is not None:
        ready &= at
    n = np.zeros(c.shape, bool)
    with np.errstate(all="ignore"):
        for a, b in ((x["close"], x["ema20"]), (x["close"], x["ema50"]),
                     (x["volume_ratio"], np.full_like(c, par["min_volume_ratio"]))):
            n |= ready & (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
        exact = [("close", x["previous_high"]), ("candle_return", par["min_candle_return"]),
                 ("candle_return", par["max_candle_return"]), ("return_1h", par["max_return_1h"]),
                 ("return_1h", par["min_return_1h"]), ("return_2h", par["min_return_2h"]),
                 ("return_6h", par["min_return_6h"]), ("extension_return", x["extension_cap"]),
                 ("range_position", par["min_range_position"]), ("upper_wick_fraction", par["max_upper_wick"])]
        for k, thr in exact:
            n |= ready & (x[k] == thr)
        # the confirmation's compares, at candles whose breakout candle (two back) passed the gate
        two_back = np.zeros_like(ready)
        two_back[:, 2:] = r["entry"][:, :-2] == 0
        if at is not None:
            two_back &= at
        c1 = np.full_like(c, np.nan)
        c1[:, 1:] = c[:, :-1]
        c2, ph2 = np.full_like(c, np.nan), np.full_like(c, np.nan)
        c2[:, 2:], ph2[:, 2:] = c[:, :-2], x["previous_high"][:, :-2]
        n |= two_back & ((c1 == ph2) | (c == c2))
    return n


def near_ties(*args, **kw) -> int:
    """How many candles near_tie_mask flags."""
    return int(near_tie_mask(*args, **kw).sum())


def injected_panel(S: int, T: int, seed: int, tile: int = 1024, nan_rate: float = 0.001):
    """Seeded quiet walks [S, T] with a breakout set-up (a gentle rise, a +6 %
    hour on four times the volume, two confirming closes, a decay) about every
    64 candles and, around every multiple of `tile`, one whose breakout candle
    falls on tile - 3 .. tile + 1 (cycling with the row): the breakout ->
    confirmation triple, the 48-high window, the 32-volume window and the
    t - 96 anchor all straddle the boundary. Some set-ups are spoiled (a failed
    confirmation, a long wick, no volume); a few NaN / zero fields; row 2 (if
    any) has a NaN close right after each tile boundary (the serial ewm path).
    A walk this long crosses its own EMAs within 1e-6 now and then: such
    candles are nudged (close by 1e-4, volume by 1e-3) until near_tie_mask is
    empty, so exact codes can be demanded of a kernel whose ewm columns agree
    to 1e-9 (tests/test_topgainer_ref.py asserts the panels are tie-free).
    Returns a dict of arrays with risk_ok."""
    g = np.random.default_rng(seed)
    r = g.normal(0.0, 0.0015, (S, T))
    vol = 10.0 ** g.uniform(1.0, 4.0, (S, 1)) * np.exp(g.normal(0.0, 0.15, (S, T)))
    spoil = {}
    for s in range(S):
        spots = list(range(100 + s % 7, T - 3, 64))
        for b in range(tile, T + tile, tile):
            at = b - 3 + s % 5
            spots = [x for x in spots if abs(x - at) >= 56]   # outside each other's 48-high lookback
            if 60 <= at < T - 3:
                spots.append(at)
        for b in sorted(spots):
            r[s, b - 24:b - 4] = 0.03 / 20 + g.normal(0.0, 0.0004, 20)
            r[s, b - 3:b] = g.uniform(0.008, 0.012, 3)
            r[s, b] = np.log(1.0 + g.uniform(0.025, 0.04))
            r[s, b + 1], r[s, b + 2] = g.uniform(0.002, 0.006), g.uniform(0.004, 0.008)
            r[s, b + 3:b + 15] = (-0.085 / 12 + g.normal(0.0, 0.0004, 12))[:T - (b + 3)]
            vol[s, b] *= g.uniform(3.5, 5.0)
            kind = int(g.integers(0, 8)) if b % tile > 8 and b % tile < tile - 8 else 0
            if kind == 1:
                r[s, b + 1] = -0.06
            elif kind == 2:
                r[s, b + 2] = -0.012
            elif kind == 3:
                vol[s, b] = vol[s, b - 1]
            elif kind == 4:
                r[s, b] = np.log(1.12)
            spoil[(s, b)] = kind
    c = 10.0 ** g.uniform(-2, 3, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    o = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    h = np.maximum(o, c) * (1.0 + g.uniform(0.0, 0.0015, (S, T)))
    l = np.minimum(o, c) * (1.0 - g.uniform(0.0, 0.0015, (S, T)))
    for (s, b), kind in spoil.items():
        if kind == 5:
            h[s, b] = c[s, b] * 1.025
        elif kind == 6 and b >= 10:
            h[s, b - 10] = c[s, b] * 1.03
    atr = c * g.uniform(0.004, 0.012, (S, T))
    qv = vol * c * g.uniform(0.98, 1.02, (S, T))
    for arr, val in ((c, np.nan), (vol, 0.0), (atr, np.nan), (o, -1.0), (qv, np.inf), (h, np.nan)):
        arr[g.random((S, T)) < nan_rate] = val
    if S > 2:
        c[2] = np.where(np.isnan(c[2]), o[2], c[2])   # the only missing closes of row 2: after the boundaries
        for b in range(tile, T, tile):
            if b + 1 < T:
                c[2, b + 1] = np.nan
    risk_ok = g.random((S, T)) >= 0.15
    for _ in range(20):
        ties = near_tie_mask(o, h, l, c, vol, qv, atr) | near_tie_mask(o, h, l, c, vol)   # both recorded runs
        if not ties.any():
            break
        c[ties] *= 1.0 + 1e-4
        vol[ties] *= 1.0 + 1e-3
    return dict(open=o, high=h, low=l, close=c, volume=vol, quote_volume=qv, atr=atr, risk_ok=risk_ok)
