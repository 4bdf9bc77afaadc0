"""Shared inputs of tests/test_meanrev_ref.py and tests/test_meanrev_gpu.py:
the fixture tests/golden/meanrev_gates.npz with its regenerated panel, seeded
panels for the kernel's 64-candle step edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import meanrev_panel_gen as pg   # noqa: E402
import meanrev_ref as ref        # noqa: E402

STEP = pg.STEP_MS
TREND_CEILING = 0.06   # max_trend_score on the seeded panels (see seeded_panel)
PANELS = ("open", "high", "low", "close", "volume", "atr", "bb_upper")


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "meanrev_gates.npz")
    fx = {k: z[k] for k in z.files}
    # previous_rsi is recorded as "the previous candle's rsi, bit for bit" (make_golden_meanrev asserts it)
    assert bool(fx["previous_rsi_is_shifted_rsi"])
    S = fx["rsi"].shape[0]
    prev = np.concatenate([np.full((S, 1), np.nan), fx["rsi"][:, :-1]], axis=1)
    prev[fx["status"] == ref.NO_FRAME] = np.nan
    prev[np.arange(S), pg.mean_reversion_panel()["first_t"]] = np.nan
    fx["previous_rsi"] = prev
    return fx


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.mean_reversion_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "meanrev_panel_gen drifted from the recorded inputs"
    return p


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


# the bars of the features formed in the pass: rsi / previous_rsi 1e-9 x 100 absolute (bq_wilder_rsi's bar in
# test_signals_gpu.py), the rolling means and trend_score 1e-9 relative, score 1e-9 absolute, stop_loss_pct bits
BARS = {"rsi": ("abs", 1e-7), "previous_rsi": ("abs", 1e-7), "volume_ma": ("rel", 1e-9), "atr_ma": ("rel", 1e-9),
        "trend_score": ("rel", 1e-9), "score": ("abs", 1e-9)}


def assert_values_close(got, want, what=""):
    """BARS; NaN exactly where the reference has NaN; stop_loss_pct bit for bit."""
    for name, (kind, tol) in BARS.items():
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert (np.isnan(g) == np.isnan(w)).all(), \
            f"{what}: {name}: NaN pattern differs at {np.argwhere(np.isnan(g) != np.isnan(w))[:5].tolist()}"
        m = ~np.isnan(w)
        err = np.abs(g[m] - w[m])
        bound = tol * np.abs(w[m]) if kind == "rel" else np.full(err.shape, tol)
        worst = np.argmax(err - bound) if err.size else 0
        print(f"{what}: {name}: max error {err.max() if err.size else 0.0:.3e}")
        assert (err <= bound).all(), f"{what}: {name}: error {err[worst]} at value {w[m][worst]} (bound {bound[worst]})"
    assert_values_bits(got, want, what, names=("stop_loss_pct",))


def assert_state_equal(got, want, what=""):
    gh, gl = (np.asarray(x) for x in got)
    wh, wl = (np.asarray(x) for x in want)
    assert (gh.astype(bool) == wh.astype(bool)).all(), f"{what}: has differs"
    m = wh.astype(bool)
    assert (gl[m] == wl[m]).all(), f"{what}: last_open_time differs"


def recorded(fx=None) -> dict:
    """The recording in replay()'s output layout; score is _score without its
    round(.., 4) on the recorded rsi (the recorded, rounded score is checked
    against it by test_meanrev_ref.py)."""
    fx = fx or fixture()
    out = {k: fx[k] for k in ref.FEATURES + ("stop_loss_pct", "status")}
    out["score"] = np.where(fx["status"] == ref.EMIT, ref.score(fx["rsi"]), np.nan)
    return out


def recorded_features(fx=None) -> dict:
    fx = fx or fixture()
    return {k: fx[k] for k in ref.FEATURES}


def no_near_ties(p: dict, want: dict, first, band=1e-7, **params) -> None:
    """No status of `want` rests on a comparison that features at the 1e-9
    bars could flip: the margins, from the restatement's own values, are
    above `band` (relative; absolute x 100 for the RSI)."""
    st = want["status"]
    S, T = st.shape
    emit = st == ref.EMIT
    P = {**ref.DEFAULTS, **params}
    ft = ref.features(p["close"], p["volume"], p["atr"], first, p.get("lens"), P)
    rsi, prsi = ft["rsi"], ft["previous_rsi"]
    o, h, l, c = (p[k] for k in ("open", "high", "low", "close"))
    with np.errstate(invalid="ignore", divide="ignore"):
        rest = (c >= p["bb_upper"]) & (c < o) & ((h - np.where(c > o, c, o)) / (h - l) >= P["min_wick_ratio"])
        at_setup = (emit | (st >= ref.NO_SETUP)) & rest

        def near(a, b, cells, scale=None):
            d = np.abs(a - b) <= band * (np.maximum(np.abs(a), np.abs(b)) if scale is None else scale)
            return int((d & cells).sum())

        ties = (near(p["atr"], P["atr_spike_max"] * ft["atr_ma"], emit | (st >= ref.ATR_SPIKE)),
                near(p["volume"], P["volume_ratio_min"] * ft["volume_ma"], emit | (st >= ref.LOW_VOLUME)),
                near(rsi, np.full((S, T), P["rsi_short_min"]), at_setup & (rsi < prsi), 100.0),
                # rsi == previous_rsi exactly: the candle after a missing close, where neither mean is updated and
                # the kernel's serial recursion carries the same bits
                near(rsi, prsi, at_setup & (rsi >= P["rsi_short_min"]) & (rsi != prsi), 100.0),
                near(ft["trend_score"], np.full((S, T), P["max_trend_score"]), emit | (st >= ref.TREND_TOO_HIGH)))
    assert not any(ties), f"near-ties (atr, volume, rsi vs 76, rsi hook, trend): {ties}: choose another seed"


def fixture_kwargs(with_features: bool) -> dict:
    """replay()'s keyword inputs on the fixture panel (numpy)."""
    p = panel()
    kw = dict(ctx_ok=p["ctx_ok"], sym=pg.sym_of(p), first_t=p["first_t"], lens=p["lens"])
    if with_features:
        kw["features_given"] = recorded_features()
    return kw


def seeded_panel(S: int, T: int, seed: int, *, first_t=None, nan_close=(), nan_volume=(), per_candle_ctx=True,
                 sym_dims=2) -> dict:
    """A random panel dense in fade setups: a drift of 4-7 falling bars, a
    burst of 2-4 bars at 1-2 %, one small red candle, over and over; bb_upper
    planted under the close at the red candles, their volume above the
    average, high == low cells, a context per candle with holes, a snapshot
    entry per cell. The closes climb by about 0.4 % a candle, which is what
    keeps the Wilder RSI above 76 at every hook; EMA 20 - EMA 50 then sits
    near 6 % of the price, so the tests on these panels pass
    max_trend_score=TREND_CEILING to have candidates on both sides of the
    ceiling. It also keeps trend_score away from a zero crossing, where its
    relative error is unbounded for any summation order; the first candles of
    a frame starting at first_t (None: 0), where both means still sit on the
    seed, are moved off zero by meanrev_panel_gen.off_zero_crossings. nan_close
    / nan_volume: (row, candle) cells set to NaN."""
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 0.0003, (S, T))
    red = np.zeros((S, T), bool)
    for s in range(S):
        t = int(rng.integers(0, 6))
        while t < T:
            drift, burst = int(rng.integers(4, 8)), int(rng.integers(2, 5))
            seg = np.concatenate([-rng.uniform(0.001, 0.003, drift), rng.uniform(0.01, 0.02, burst),
                                  [-rng.uniform(0.0008, 0.0015)]])
            n = min(len(seg), T - t)
            r[s, t:t + n] += seg[:n]
            if t + len(seg) - 1 < T:
                red[s, t + len(seg) - 1] = True
            t += len(seg)
    close = 10.0 ** rng.uniform(-1, 2, (S, 1)) * np.exp(np.cumsum(r, axis=1))
    pg.off_zero_crossings(close, np.zeros(S, np.int64) if first_t is None else np.minimum(first_t, T - 1))
    opn = np.concatenate([close[:, :1] * 1.0003, close[:, :-1]], axis=1)
    high = np.maximum(opn, close) * (1 + rng.uniform(0.0001, 0.002, (S, T)))
    low = np.minimum(opn, close) * (1 - rng.uniform(0.0001, 0.002, (S, T)))
    volume = rng.lognormal(3, 0.3, (S, T))
    volume[red] = np.exp(3.0) * rng.uniform(1.3, 2.5, (S, T))[red]
    atr = close * 0.0035 * rng.uniform(0.9, 1.1, (S, T))
    atr[rng.random((S, T)) < 0.03] *= 3.0
    atr[rng.random((S, T)) < 0.05] *= 2.3      # stop_loss_pct past its cap
    bb = close * (1 + rng.uniform(0.0005, 0.01, (S, T)))
    bb[red] = (close * (1 - rng.uniform(0.0005, 0.003, (S, T))))[red]
    flat = rng.random((S, T)) < 0.02
    high[flat] = low[flat]
    Tc = T if per_candle_ctx else 1
    ctx = np.stack([rng.uniform(0.02, 0.2, Tc), np.full(Tc, 0.2), np.full(Tc, 0.3), rng.uniform(-0.5, 0.1, Tc),
                    rng.normal(0.0, 0.004, Tc)])
    k = rng.random(Tc)
    ctx[0][k < 0.08] = 0.6
    ctx[1][(k >= 0.08) & (k < 0.16)] = 0.5
    ctx[3][(k >= 0.16) & (k < 0.24)], ctx[4][(k >= 0.16) & (k < 0.24)] = 0.4, 0.002
    shape = (S, T) if sym_dims == 2 else (S,)
    kind = rng.choice(5, size=shape, p=[0.2, 0.5, 0.1, 0.1, 0.1])
    sym = dict(ok=kind != 0, atr_pct=np.where(kind == 2, 0.05, rng.uniform(0.004, 0.028, shape)),
               trend_score=np.where(kind == 4, 0.004, rng.normal(-0.002, 0.001, shape)),
               micro_regime=np.where(kind == 4, pg.TREND_UP, pg.RANGE).astype(np.uint8),
               micro_transition=np.where(kind == 3, pg.BREAKOUT_UP, pg.NONE).astype(np.uint8))
    p = dict(open=opn, high=high, low=low, close=close, volume=volume, atr=atr, bb_upper=bb,
             open_time=np.tile(pg.T0_MS + np.arange(T, dtype=np.int64) * STEP, (S, 1)), ctx=ctx,
             ctx_ok=rng.random(Tc) > 0.08, sym=sym)
    for s, t in nan_close:
        if s < S and t < T:
            p["close"][s, t] = np.nan
    for s, t in nan_volume:
        if s < S and t < T:
            p["volume"][s, t] = np.nan
    return p


def random_features(p: dict, seed: int) -> dict:
    """Feature columns dense in setups for the point-wise variant, with NaN cells."""
    rng = np.random.default_rng(seed)
    S, T = p["close"].shape
    rsi = rng.uniform(70, 95, (S, T))
    ft = dict(rsi=rsi, previous_rsi=rsi + rng.normal(1.0, 2.0, (S, T)),
              volume_ma=np.nan_to_num(p["volume"], nan=20.0) * rng.uniform(0.7, 1.4, (S, T)),
              atr_ma=p["atr"] * rng.uniform(0.4, 1.3, (S, T)), trend_score=rng.normal(0.05, 0.02, (S, T)))
    for k in ft:
        ft[k][rng.random((S, T)) < 0.02] = np.nan
    return ft


def ref_replay(p: dict, **kw):
    return ref.replay(*(p[k] for k in PANELS), p["open_time"], p["ctx"], p.get("ctx_ok"), sym=p.get("sym"), **kw)
