"""The bar of the stress-row parity tests, and their pandas side.

The project's constants (tests/util.py: RTOL 1e-9, ATOL_REL 1e-11) with a
LOCAL scale in place of the row mean — on a row that falls 100x a row-mean
scale leaves the small-price part a 100x looser absolute term:

  price-unit columns   scale[t] = max |open|, |high|, |low|, |close| over
                       [t - 127, t]: MAX_WINDOW (126) plus the neighbouring
                       candle of the deltas / true range
  EMA family           the larger of that and ema50(|close|)[t] in long double
                       (an EMA remembers a crash for longer than 127 candles)
  rsi, mfi, Wilder RSI, ADX    100
  z-score              1

  err(x) = |x - exact|,  bar = RTOL |exact| + ATOL_REL scale

exact is tests/exact_ref.py. A kernel is held to
err(kernel) <= max(bar, err(pandas)): to the exact value, except where pandas
itself is outside the bar — and where that happens is pinned, pair by pair, by
tests/test_stress_ref.py.
"""

from __future__ import annotations

import numpy as np
import pandas as pd
from numpy.lib.stride_tricks import sliding_window_view

from tests import exact_ref
from tests.util import ATOL_REL, RTOL

LD = np.longdouble
REACH = 128   # candles [t - 127, t]
EMA_FAMILY = ("ema20", "ema50", "macd", "macd_signal")
HUNDRED = ("rsi", "mfi", "wilder_rsi", "adx")


def local_scale(panel) -> np.ndarray:
    """[S, T] max |open|, |high|, |low|, |close| over [t - 127, t]."""
    m = np.max(np.abs(np.stack([panel[k] for k in ("open", "high", "low", "close")])), axis=0)
    pad = np.concatenate([np.zeros((m.shape[0], REACH - 1)), m], axis=1)
    return sliding_window_view(pad, REACH, axis=-1).max(axis=-1)


def ema_scale(panel, span: int = 50) -> np.ndarray:
    e = exact_ref.ema(np.abs(np.asarray(panel["close"], dtype=LD)), exact_ref.span_alpha(span))
    return np.maximum(local_scale(panel).astype(LD), e)


def scales(panel, ema_span: int = 50) -> dict:
    """name -> scale (scalar or [S, T]) for every compared quantity."""
    loc = local_scale(panel)
    es = ema_scale(panel, ema_span)
    out = {k: loc for k in exact_ref.CANONICAL}
    out.update({k: es for k in EMA_FAMILY})
    out.update({k: 100.0 for k in HUNDRED})
    out["zscore"] = 1.0
    return out


def bar(exact, scale) -> np.ndarray:
    return LD(RTOL) * np.abs(exact) + LD(ATOL_REL) * np.asarray(scale, dtype=LD)


def err(x, exact) -> np.ndarray:
    """|x - exact| in long double; 0 where both are NaN or the same infinity."""
    x = np.asarray(x, dtype=LD)
    with np.errstate(invalid="ignore"):
        e = np.abs(x - exact)
    same = (np.isnan(x) & np.isnan(exact)) | (np.isinf(x) & (x == exact))
    return np.where(same, LD(0), e)


def outside(x, exact, scale) -> np.ndarray:
    """Boolean map of the candles where x is outside the bar around exact
    (a NaN against a number counts as outside, NaN against NaN as inside)."""
    both = np.isnan(np.asarray(x, dtype=LD)) & np.isnan(exact)
    return ~((err(x, exact) <= bar(exact, scale)) | both)


def ratio(x, exact, scale) -> np.ndarray:
    """err / bar (float64; 0 where both NaN)."""
    b = bar(exact, scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = err(x, exact) / np.where(np.isnan(b), LD(1), b)
    return np.asarray(r, dtype=np.float64)


def assert_nan_pattern(got, want, name: str):
    bad = np.isnan(np.asarray(got, dtype=np.float64)) != np.isnan(np.asarray(want, dtype=np.float64))
    assert not bad.any(), f"{name}: NaN pattern differs at {np.argwhere(bad)[:5].tolist()} ({int(bad.sum())} candles)"


def assert_held(got, exact, pandas_val, scale, name: str, rows=None):
    """NaN pattern equal to pandas'; err(got) <= max(bar, err(pandas)) at every
    candle. Returns the worst err(got) / bar per row (what DESIGN.md records)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(exact) == np.shape(pandas_val), f"{name}: shapes {got.shape} {np.shape(exact)}"
    assert_nan_pattern(got, pandas_val, name)
    eg, ep, b = err(got, exact), err(pandas_val, exact), bar(exact, scale)
    lim = np.fmax(np.broadcast_to(b, eg.shape), ep)
    bad = ~((eg <= lim) | np.isnan(exact))   # NaN candles: the pattern assertion above
    if bad.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bad, np.nan_to_num(np.asarray(eg / lim, dtype=np.float64), nan=np.inf), 0.0)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        row = rows[i[0]] if rows is not None and len(rows) == got.shape[0] else ""
        raise AssertionError(
            f"{name}: {int(bad.sum())} candles outside max(bar, err(pandas)); worst at {tuple(int(j) for j in i)} {row}: "
            f"got {got[i]!r} exact {float(exact[i])!r} pandas {float(np.asarray(pandas_val)[i])!r} "
            f"err {float(eg[i]):.3e} bar {float(np.broadcast_to(b, eg.shape)[i]):.3e} err(pandas) {float(ep[i]):.3e}")
    return ratio(got, exact, scale)


def cut_sides(value, exact, cut: float, scale) -> np.ndarray:
    """The candles at which a threshold decision is compared: every candle
    with a value, except where the exact reference lies within its own bar of
    the cut (there either side is a correct rounding)."""
    with np.errstate(invalid="ignore"):
        return ~np.isnan(np.asarray(value, dtype=np.float64)) & (np.abs(exact - LD(cut)) > bar(exact, scale))


def assert_same_side(fast, replay, exact, cut: float, scale, name: str):
    """The fast and the exact=True form agree on the side of `cut`."""
    m = cut_sides(replay, exact, cut, scale)
    bad = m & ((np.asarray(fast) > cut) != (np.asarray(replay) > cut))
    assert not bad.any(), f"{name}: sides differ at {np.argwhere(bad)[:5].tolist()} ({int(bad.sum())} candles)"
    return int(m.sum())


# ---- the pandas side of the signal helpers ----------------------------------------

def pandas_wilder_rsi(close, window: int = 14) -> np.ndarray:
    out = []
    for row in np.atleast_2d(close):
        delta = pd.Series(row).diff()
        ag = delta.clip(lower=0).ewm(alpha=1 / window, min_periods=window, adjust=False).mean()
        al = (-delta.clip(upper=0)).ewm(alpha=1 / window, min_periods=window, adjust=False).mean()
        den = ag + al
        out.append((100 * ag / den).where(den != 0, 50.0).to_numpy())
    return np.stack(out)


def pandas_adx(high, low, close, window: int = 14) -> np.ndarray:
    """_compute_adx on every prefix frame: its rolling sums and means do not
    look ahead, so the whole-row series holds every prefix's last value."""
    out = []
    for hr, lr, cr in zip(np.atleast_2d(high), np.atleast_2d(low), np.atleast_2d(close)):
        h, l, c = pd.Series(hr), pd.Series(lr), pd.Series(cr)
        hd, ld = h.diff(), -l.diff()
        plus = hd.where((hd > ld) & (hd > 0), 0.0)
        minus = ld.where((ld > hd) & (ld > 0), 0.0)
        pc = c.shift(1)
        tr = pd.concat([h - l, (h - pc).abs(), (l - pc).abs()], axis=1).max(axis=1)
        atr_sum = tr.rolling(window, min_periods=window).sum()
        pdi = 100.0 * plus.rolling(window, min_periods=window).sum() / atr_sum
        mdi = 100.0 * minus.rolling(window, min_periods=window).sum() / atr_sum
        tot = pdi + mdi
        dx = (100.0 * (pdi - mdi).abs() / tot.where(tot != 0, float("nan"))).fillna(0.0)
        out.append(dx.rolling(window, min_periods=window).mean().fillna(100.0).to_numpy())
    return np.stack(out)


def pandas_zscore(close, window: int = 20) -> np.ndarray:
    out = []
    for row in np.atleast_2d(close):
        c = pd.Series(row)
        m = c.rolling(window, min_periods=window).mean()
        sd = c.rolling(window, min_periods=window).std(ddof=0)
        z = ((c - m) / sd).where(~((sd == 0) | sd.isna()), 0.0)
        out.append(z.to_numpy())
    return np.stack(out)


# ---- the rows with their three sides, computed once per session -------------------

# the non-default parameters of test_enrich_gpu.test_subset_of_columns_and_params:
# the generic (not unrolled) instantiation of the window walks
OTHER_PARAMS = dict(ma_periods=(5, 30, 126), rsi_window=9, bb_window=10, bb_ddof=0, bb_k=2.5, atr_window=21,
                    twap_window=8, ema_spans=(9, 34), mfi_window=10, macd_fast=8, macd_slow=21, macd_signal=5)
OTHER_COLUMNS = ("ma_7", "ma_100", "rsi", "bb_upper", "bb_lower", "ATR", "mfi", "macd_signal", "ema50")
SLOT_TO_ORACLE = {"ma_7": "ma_{0}", "ma_25": "ma_{1}", "ma_100": "ma_{2}", "ema20": "ema{3}", "ema50": "ema{4}"}


BB = ("bb_upper", "bb_lower")
PANDAS_OUTSIDE = {
    # kind -> {(family, quantity): largest share of the row's candles where pandas is outside the
    # bar}: measured and pinned by tests/test_stress_ref.py (figures in its docstring); nowhere else
    # may a GPU test fall back on err(pandas)
    "default": {("ramp_down", k): 0.50 for k in BB} | {("crash100@1024", k): 0.58 for k in BB}
    | {("ramp_down", "zscore"): 0.62, ("crash100@1024", "zscore"): 0.58, ("crash10@1024", "zscore"): 0.58,
       ("crash10@700", "zscore"): 0.72, ("pump_dump", "zscore"): 0.63},
    "other": {("ramp_down", k): 0.60 for k in BB} | {("crash100@1024", k): 0.58 for k in BB}
    | {("crash10@1024", k): 0.01 for k in BB},
    "long": {},
}


def pandas_enrich(panel, p: dict | None = None) -> dict[str, np.ndarray]:
    """oracle enrich_panel under the canonical slot names whatever the periods."""
    from oracle import indicators_ref as ref

    if not p:
        return ref.enrich_panel(*(panel[k] for k in ("open", "high", "low", "close", "volume")))
    q = {**ref.DEFAULTS, **p}
    ids = (*q["ma_periods"], *q["ema_spans"])
    out = {k: [] for k in exact_ref.CANONICAL}
    for s in range(panel["close"].shape[0]):
        df = pd.DataFrame({k: panel[k][s] for k in ("open", "high", "low", "close", "volume")})
        df = ref.indicators_enrichment(df, q)
        for k in exact_ref.CANONICAL:
            out[k].append(df[SLOT_TO_ORACLE.get(k, k).format(*ids)].to_numpy())
    return {k: np.stack(v) for k, v in out.items()}


class Sides:
    """One set of stress rows: the panel, the long-double values, pandas'
    values and the scales of every enrich column and signal helper."""

    def __init__(self, fams, p: dict | None = None):
        from tests import stress_cases

        self.fams = fams
        self.names = stress_cases.names(fams)
        self.panel = stress_cases.panel(fams)
        P = self.panel
        self.exact = exact_ref.enrich(*(P[k] for k in stress_cases.FIELDS), p)
        self.pandas = pandas_enrich(P, p)
        self.scale = scales(P)
        for d in (self.exact, self.pandas, self.scale):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)

    def row(self, name: str) -> int:
        return self.names.index(name)

    def signal_sides(self):
        """name -> (exact, pandas) of the three signal helpers at their default windows."""
        P = self.panel
        return {
            "wilder_rsi": (exact_ref.wilder_rsi(P["close"]), pandas_wilder_rsi(P["close"])),
            "adx": (exact_ref.adx(P["high"], P["low"], P["close"]), pandas_adx(P["high"], P["low"], P["close"])),
            "zscore": (exact_ref.zscore(P["close"]), pandas_zscore(P["close"])),
        }


_SIDES: dict = {}


def sides(kind: str = "default") -> Sides:
    """'default': the 17 families at T = 2300, default parameters; 'other':
    the same rows under OTHER_PARAMS; 'long': the T = 4100 rows."""
    from tests import stress_cases

    if kind not in _SIDES:
        if kind == "default":
            _SIDES[kind] = Sides(stress_cases.families())
        elif kind == "other":
            _SIDES[kind] = Sides(stress_cases.families(), OTHER_PARAMS)
        elif kind == "long":
            _SIDES[kind] = Sides(stress_cases.long_families())
        else:
            raise KeyError(kind)
    return _SIDES[kind]


def pandas_outside_pairs(s: Sides, quantities: dict) -> dict:
    """(family, name) -> (worst err(pandas) / bar, share of candles outside)
    for every pair where pandas leaves the bar; quantities maps a name to
    (exact, pandas, scale)."""
    out = {}
    for k, (ex, pdv, sc) in quantities.items():
        o = outside(pdv, ex, sc)
        r = ratio(pdv, ex, sc)
        for i, n in enumerate(s.names):
            if o[i].any():
                out[(n, k)] = (float(np.nanmax(r[i])), float(o[i].mean()))
    return out


# ---- market features (the 400-bar store cap) ----------------------------------------

FEATURES = ("return_pct", "ema20", "ema50", "trend_score", "atr_pct", "bb_width")
# (family, feature) -> candles at which pandas (market_ref.panel_features_at) is outside
# test_market_gpu's rule around the long-double restatement, among feature_candles():
# measured and pinned by tests/test_stress_ref.py; only here may the kernel differ from pandas
FEATURE_PANDAS_OUTSIDE = {("crash10@700", "bb_width"): 8, ("crash10@1024", "bb_width"): 8,
                          ("crash100@1024", "bb_width"): 8, ("pump_dump", "bb_width"): 2}


def feature_rule(x: float, y: float) -> bool:
    """test_market_gpu's bar: rtol 1e-9, scale 1e-3."""
    return abs(x - y) <= RTOL * abs(y) + ATOL_REL * 1e-3


def feature_candles(s: Sides):
    """(row, t): [event - 2, event + 26] of every crash and spike row, the cap
    edge [398, 402] of every row, and the plateau edges with the candles at
    which the 20-candle window fills with and empties of the plateau."""
    out = set()
    for i, f in enumerate(s.fams):
        out |= {(i, t) for t in range(398, 403)}
        if f.name.startswith(("crash", "spike")):
            out |= {(i, t) for e in f.events for t in range(e - 2, e + 27)}
        for a, b in f.plateaus:
            out |= {(i, t) for x in (a, b) for t in (x - 2, x - 1, x, x + 1, x + 18, x + 19, x + 20)}
    return sorted(out)


def features_exact(h, l, c, t, max_bars=400) -> dict:
    """The long-double features of one row at one candle, rounded once."""
    return {k: float(v[0]) for k, v in exact_ref.market_features_at(h, l, c, t, max_bars).items()}
