"""Shared inputs of tests/test_rsreversal_ref.py, tests/test_rsreversal_gpu.py
and tests/test_rsreversal_cohort_gpu.py: the fixture
tests/golden/rsreversal_gates.npz with its regenerated panel, the hand-built
cases for the kernel's 64-candle step edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import rsreversal_panel_gen as pg   # noqa: E402
import rsreversal_ref as ref        # noqa: E402

CTX = ("context_ok", "market_regime", "average_return", "features_ok", "rs")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "rsreversal_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    """The fixture's inputs in replay()'s argument names (computed once; do not modify)."""
    p = pg.rsr_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "rsreversal_panel_gen drifted from the recorded inputs"
    return dict(p, context_ok=pg.context_ok(p), features_ok=pg.features_ok(p))


def recorded() -> dict:
    fx = fixture()
    return {k: fx[k] for k in ("status",) + ref.VALUES}


def ref_replay(p: dict, **kw):
    return ref.replay(p["volume"], *(p[k] for k in CTX), **kw)


@functools.lru_cache(maxsize=2)
def fixture_replay(rolling: bool = False):
    """The restatement on the fixture panel (computed once; do not modify)."""
    p = panel()
    return ref_replay(p, first_t=p["first_t"], lens=p["lens"],
                      floor=ref.rolling_quantile if rolling else ref.series_quantile)


def same_value(a, b) -> np.ndarray:
    """Element-wise: both NaN, or equal (a zero's sign is free: np.sort and
    the kernel's key order may pick either of two equal zeros)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a == b)


def assert_codes_equal(got, want, what=""):
    g, w = np.asarray(got["status"]), np.asarray(want["status"])
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: status differs at {bad[:5].tolist()}: " \
                          f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"


def assert_values_equal(got, want, what="", names=ref.VALUES):
    for name in names:
        bad = np.argwhere(~same_value(got[name], want[name]))
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: " \
                              f"{[(got[name][tuple(i)], want[name][tuple(i)]) for i in bad[:5]]}"


FIRSTS = (0, 31, 63, 64)


def edge_rows(S, T):
    """first_t cycling over 0 / 31 / 63 / 64; the last row of three or more has lens = T - 2 (rows 0 and 1 hold
    the NaN planted from the newest candle)."""
    first = np.array([FIRSTS[s % 4] for s in range(S)]).clip(0, max(T - 1, 0))
    lens = np.full(S, T)
    if S > 2:
        lens[S - 1] = max(T - 2, 1)
    return first, lens


def edge_panel(S: int, T: int, seed: int, window: int = 96, through: str = "most", ctx_T: int | None = None,
               per_cell: bool = True) -> dict:
    """Volumes rounded to one decimal (ties with the floor), dense in what the
    kernel can get wrong: scattered NaN, +inf, -inf and zero volumes, a run of
    +inf that fills most of a window, a NaN and an infinity on lanes 63 and 0
    of a step, and a NaN exactly `window` candles (row 0: outside the newest
    window) and `window - 1` candles (row 1: inside) before the newest candle.
    through: the share of candles whose context passes the route: "most",
    "none", "all", or "steps" (alternating per 64-candle step). ctx_T: 1 or T
    (default T); per_cell: features_ok / rs [S, T], else [S]."""
    rng = np.random.default_rng(seed)
    vol = np.round(10.0 ** rng.uniform(0.5, 2.0, (S, 1)) * np.exp(rng.normal(0.0, 0.6, (S, T))), 1)
    u = rng.random((S, T))
    vol[u < 0.02] = np.nan
    vol[(u >= 0.02) & (u < 0.03)] = np.inf
    vol[(u >= 0.03) & (u < 0.035)] = -np.inf
    vol[(u >= 0.035) & (u < 0.06)] = 0.0
    if S > 2 and T > 40:
        a = int(rng.integers(0, T // 3))
        vol[2, a:a + max(int(0.8 * window), 1)] = np.inf
    if S > 3 and T > 70:
        vol[3, 63], vol[3, 64] = np.nan, np.inf
    last = T - 1
    for s, t in ((0, last - window), (1, last - window + 1)):
        if s < S and 0 <= t < T:
            vol[s, max(t - 3, 0):t + 4] = np.round(rng.uniform(5, 50, len(vol[s, max(t - 3, 0):t + 4])), 1)
            vol[s, t] = np.nan
    Tc = T if ctx_T is None else ctx_T
    if through == "none":
        mk = rng.choice([-1, 0, 1, 3, 4], Tc).astype(np.int8)
        ok = rng.random(Tc) < 0.8
        ar = rng.uniform(-0.08, 0.03, Tc)
    elif through == "all":
        mk, ok, ar = np.full(Tc, ref.RANGE, np.int8), np.ones(Tc, bool), rng.uniform(-0.08, -0.021, Tc)
    else:
        mk = rng.choice([-1, 0, 1, 2, 3, 4], Tc, p=[0.04, 0.03, 0.03, 0.84, 0.03, 0.03]).astype(np.int8)
        ok = rng.random(Tc) < 0.9
        ar = np.where(rng.random(Tc) < 0.9, rng.uniform(-0.08, -0.021, Tc), rng.uniform(-0.02, 0.03, Tc))
        ar[rng.random(Tc) < 0.04] = np.nan
        ar[rng.random(Tc) < 0.03] = -0.02
        if through == "steps" and Tc > 1:
            mk[(np.arange(Tc) // 64) % 2 == 0] = 0
    shape = (S, T) if per_cell else (S,)
    fok = rng.random(shape) < 0.9
    rs = np.where(rng.random(shape) < 0.85, rng.uniform(0.051, 0.4, shape), rng.uniform(-0.2, 0.05, shape))
    rs[rng.random(shape) < 0.04] = np.nan
    rs[rng.random(shape) < 0.03] = 0.05
    if through == "all":
        fok, rs = np.ones(shape, bool), rng.uniform(0.051, 0.4, shape)
    return dict(volume=vol, context_ok=ok, market_regime=mk, average_return=ar, features_ok=fok, rs=rs)
