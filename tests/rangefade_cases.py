"""Shared inputs of tests/test_rangefade_ref.py and tests/test_rangefade_gpu.py:
the fixture tests/golden/rangefade_gates.npz with its regenerated panel, small
seeded panels for the kernel's 64-candle step edges, and the comparisons."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import rangefade_panel_gen as pg   # noqa: E402
import rangefade_ref as ref        # noqa: E402

PANELS = ("open", "high", "low", "close", "volume", "rsi", "bb_upper", "bb_mid", "bb_lower")
ZSCORE_MAX_CASES = 8   # make_golden_rangefade.check_coverage shows the recording needs no more (it needs 0)


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(GOLDEN / "rangefade_gates.npz")
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=1)
def panel():
    p = pg.range_fade_panel()
    assert pg.digest(p) == str(fixture()["digest"]), "rangefade_panel_gen drifted from the recorded inputs"
    return p


def recorded(fx=None) -> dict:
    fx = fx or fixture()
    return {k: fx[k] for k in ref.VALUES + ("status",)}


def recorded_features(fx=None) -> dict:
    """The method's own adx / zscore where it computed them; elsewhere (the
    method returned before) the restatement's, which the gates do not read."""
    fx = fx or fixture()
    p = panel()
    own = ref.features(p["high"], p["low"], p["close"], p["first_t"], p["lens"])
    return {k: np.where(np.isnan(fx[k]), own[k], fx[k]) for k in ref.FEATURES}


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


def assert_values_close(got, want, close, what=""):
    """The bars of the features formed in the pass: adx 1e-9 relative plus
    1e-11 x 100 absolute (bq_adx's bar in test_signals_gpu.py), score 1e-9
    relative, zscore 1e-9 relative or, on at most ZSCORE_MAX_CASES cells,
    closer than pandas to the exactly computed value
    (indicators_ref.exact_zscore); direction bit for bit; NaN exactly where
    the reference has NaN."""
    from oracle.indicators_ref import exact_zscore
    from tests.util import assert_close, assert_close_or_exact

    for name in ("adx", "score", "zscore"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        with np.errstate(invalid="ignore"):
            err = np.nanmax(np.abs(g - w)) if (~np.isnan(w)).any() else 0.0
        print(f"{what}: {name}: max error {err:.3e}")
    assert_close(got["adx"], want["adx"], f"{what}: adx", rtol=1e-9, scale=100.0)
    assert_close(got["score"], want["score"], f"{what}: score", rtol=1e-9)
    nan = np.isnan(np.asarray(got["zscore"])) != np.isnan(np.asarray(want["zscore"]))
    assert not nan.any(), f"{what}: zscore: NaN pattern differs at {np.argwhere(nan)[:5].tolist()}"
    assert_close_or_exact(got["zscore"], want["zscore"], close, ref.DEFAULTS["zscore_window"], exact_zscore,
                          f"{what}: zscore", max_cases=ZSCORE_MAX_CASES)
    assert_values_bits(got, want, what, names=("direction",))


# ---- small seeded panels --------------------------------------------------------------------------------------
def seeded_panel(S, T, seed, first_t=None, per_candle_ctx=True, sym_dims=2, nans=(), warm=22, every=5):
    """A panel dense in setups: a rejection candle of alternating side every
    `every` candles from frame row `warm` on, mostly good contexts and
    snapshot entries. nans: (column, row, candle) cells set to NaN where they
    exist."""
    rng = np.random.default_rng(seed)
    first = np.zeros(S, np.int64) if first_t is None else np.asarray(first_t, np.int64)
    x = np.zeros((S, T))
    e = rng.normal(0.0, 0.0022, (S, T))
    for t in range(1, T):
        x[:, t] = 0.9 * x[:, t - 1] + e[:, t]
    close = 10.0 ** rng.uniform(-2, 3, (S, 1)) * np.exp(x)
    opn = np.concatenate([close[:, :1] * 1.0003, close[:, :-1]], axis=1) * (1 + rng.normal(0, 0.0002, (S, T)))
    high = np.maximum(opn, close) * (1 + rng.uniform(0.0002, 0.002, (S, T)))
    low = np.minimum(opn, close) * (1 - rng.uniform(0.0002, 0.002, (S, T)))
    volume = rng.lognormal(3, 0.45, (S, T))
    rsi = rng.uniform(22.0, 78.0, (S, T))
    planted = {}
    for s in range(S):
        for i, t in enumerate(range(int(first[s]) + warm + s % 3, T, every)):
            w = close[s, t - 19:t]
            side = (i + s) % 2
            sign = -1.0 if side == 0 else 1.0
            c = w.mean() + sign * 5.0 * w.std()
            r = 0.006 * c
            close[s, t], opn[s, t] = c, c + sign * 0.1 * r
            if side == 0:
                low[s, t], high[s, t] = c - 0.8 * r, c + 0.2 * r
            else:
                high[s, t], low[s, t] = c + 0.8 * r, c - 0.2 * r
            rsi[s, t] = (25.0 if side == 0 else 75.0) + rng.uniform(-6, 6)
            planted[(s, t)] = side
    mid = np.full((S, T), np.nan)
    up, lo = mid.copy(), mid.copy()
    for t in range(T):
        w = close[:, max(t - 19, 0):t + 1]
        mid[:, t] = w.mean(axis=1) * (1 + 5e-5)
        up[:, t], lo[:, t] = mid[:, t] + 2.0 * w.std(axis=1), mid[:, t] - 2.0 * w.std(axis=1)
    for (s, t), side in planted.items():
        if side == 0:
            lo[s, t], mid[s, t] = low[s, t] * 1.0007, close[s, t] * 1.005
        else:
            up[s, t], mid[s, t] = high[s, t] * 0.9993, close[s, t] * 0.995
    for s in range(S):   # one candle without a range
        if T > 30:
            t = int(rng.integers(25, T))
            high[s, t] = low[s, t]

    Tc = T if per_candle_ctx else 1
    kind = rng.choice(6, size=Tc, p=[0.75, 0.05, 0.05, 0.05, 0.05, 0.05]) if per_candle_ctx else np.zeros(1, int)
    ctx = np.empty((3, Tc))
    ctx[0], ctx[1], ctx[2] = 0.0, rng.uniform(0.02, 0.3, Tc), float(ref.RANGE)
    ctx[0][kind == 2] = 1.0
    ctx[1][kind == 3] = 0.5
    ctx[2][kind == 4] = ref.NONE
    ctx[2][kind == 5] = 0.0
    ctx_ok = kind != 1
    shp = (S, T) if sym_dims == 2 else (S,)
    sk = rng.choice(6, size=shp, p=[0.75, 0.05, 0.05, 0.05, 0.05, 0.05]) if sym_dims == 2 else np.zeros(S, int)
    sym = dict(ok=sk != 1, micro_regime=np.full(shp, ref.RANGE, np.uint8),
               micro_transition=rng.choice(np.array([ref.NONE, 3, 4], np.uint8), size=shp),
               atr_pct=rng.uniform(0.004, 0.035, shp), bb_width=rng.uniform(0.01, 0.07, shp))
    sym["micro_regime"][sk == 2] = ref.NONE
    sym["micro_transition"][sk == 3] = 2
    sym["atr_pct"][sk == 4] = 0.06
    sym["bb_width"][sk == 5] = 0.12
    p = dict(open=opn, high=high, low=low, close=close, volume=volume, rsi=rsi, bb_upper=up, bb_mid=mid, bb_lower=lo,
             ctx=ctx, ctx_ok=ctx_ok, sym=sym, first_t=first)
    for col, s, t in nans:
        if s < S and t < T:
            p[col][s, t] = np.nan
    return p


def ref_replay(p, **kw):
    return ref.replay(*(p[k] for k in PANELS), p["ctx"], p.get("ctx_ok"), sym=p.get("sym"), **kw)


def no_near_ties(want, band=1e-7, **params) -> None:
    """No status of `want` rests on a compare of adx or zscore that values at
    the 1e-9 bar could turn (the seeded panels are fixed: this checks them)."""
    P = {**ref.DEFAULTS, **params}
    with np.errstate(invalid="ignore"):
        for name, cuts in (("adx", (P["adx_max"],)), ("zscore", (P["long_zscore_max"], P["short_zscore_min"]))):
            for cut in cuts:
                near = np.abs(want[name] - cut) <= band * abs(cut)
                assert not near.any(), f"{name} within {band} of {cut} at {np.argwhere(near)[:3].tolist()}"
