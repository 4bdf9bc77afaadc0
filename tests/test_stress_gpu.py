"""GPU parity on trends, crashes and tick-size prices (tests/stress_cases.py).

Every kernel of the indicator hot path — bq_enrich at the default and at the
generic parameters, the tick path's ring, the time-parallel signal helpers
and their replay form, bq_market_features — on rows that trend for 2300
candles, gap by x0.1 .. x100 in one candle, sit on a tick grid and change
volume regime by 1e4. The rule (tests/stress_bar.py):

    NaN pattern == pandas'
    |kernel - exact| <= max(bar, |pandas - exact|)      at every candle

with exact the long-double restatement of tests/exact_ref.py and bar the
project's 1e-9 |exact| + 1e-11 scale under a LOCAL scale (the largest price
of the last 128 candles; 100 for the oscillators; 1 for the z-score). The
err(pandas) term is more than the bar only on the pairs that
tests/test_stress_ref.py pins; no test here uses a row-mean scale or leaves
a candle out.

Each test prints its worst err / bar per family (lines starting 'stress:'),
the figures of DESIGN.md's table.
"""

import numpy as np
import pytest
import torch

from binquant_amd import engine
from binquant_amd._lib import FEATURE_COLUMNS
from binquant_amd.synth import numpy_panel
from oracle import indicators_ref as ref
from oracle import market_ref
from tests import exact_ref, stress_bar as sb, stress_cases

pytestmark = pytest.mark.gpu

FIELDS = stress_cases.FIELDS
COLS = exact_ref.CANONICAL
PLATEAU_COLUMNS = (("ma_7", 0), ("ma_25", 1), ("ma_100", 2), ("bb_mid", None), ("bb_upper", None), ("bb_lower", None))


def _dev(panel):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in panel.items()}


def _enrich(panel, params=None, columns=COLS):
    d = _dev(panel)
    out = engine.enrich(*(d[k] for k in FIELDS), params=params, columns=columns)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _report(what, names, worst):
    """worst: column -> [S] worst err / bar per family."""
    for k, r in worst.items():
        print(f"stress: {what} {k}: " + " ".join(f"{n}={x:.3g}" for n, x in zip(names, r)))


def _check_enrich(s: sb.Sides, got, columns, what):
    worst = {}
    for k in columns:
        r = sb.assert_held(got[k], s.exact[k], s.pandas[k], s.scale[k], f"{what}.{k}", s.names)
        worst[k] = np.nanmax(np.where(np.isnan(r), 0.0, r), axis=1)
    _report(what, s.names, worst)


def _check_plateaus(s: sb.Sides, got, columns, periods, bb_window):
    """Past a plateau's warm-up the same-value rule makes the means and the
    bands the plateau price itself, in pandas and in the kernel."""
    p = s.row("tick2_plateau")
    checked = 0
    for a, b in s.fams[p].plateaus:
        price = s.fams[p].close[a]
        for k, slot in PLATEAU_COLUMNS:
            w = bb_window if slot is None else periods[slot]
            if k not in columns or a + w - 1 >= b:
                continue
            sl = slice(a + w - 1, b)
            np.testing.assert_array_equal(s.pandas[k][p, sl], price, err_msg=f"pandas {k} on plateau {a}")
            np.testing.assert_array_equal(got[k][p, sl], s.pandas[k][p, sl], err_msg=f"{k} on plateau [{a}, {b})")
            checked += 1
    assert checked >= 8


def test_enrich_every_column(cuda):
    """engine.enrich at the default parameters: all 14 columns of all 17
    families held to the exact value; the plateau means and bands and the
    ramps' RSI / MFI bit for bit; two numpy_panel rows of the same launch
    bit-equal to a launch of theirs alone."""
    s = sb.sides("default")
    S = len(s.names)
    clean = numpy_panel(2, 2300, seed0=41)
    both = {k: np.concatenate([s.panel[k], clean[k]]) for k in FIELDS}
    got = _enrich(both)
    _check_enrich(s, {k: v[:S] for k, v in got.items()}, COLS, "enrich")
    _check_plateaus(s, got, COLS, (7, 25, 100), 20)
    up, dn = s.row("ramp_up"), s.row("ramp_down")
    for i, val in ((up, 100.0), (dn, 0.0)):
        f = s.fams[i]
        tp = (f.high + f.low + f.close) / 3
        assert (np.diff(tp) > 0).all() if i == up else (np.diff(tp) < 0).all()   # the typical price is monotone
        for k in ("rsi", "mfi"):
            np.testing.assert_array_equal(s.pandas[k][i, 13:], val, err_msg=f"pandas {k} on {f.name}")
            np.testing.assert_array_equal(got[k][i], s.pandas[k][i], err_msg=f"{k} on {f.name}")
    alone = _enrich(clean)
    for k in COLS:
        np.testing.assert_array_equal(got[k][S:], alone[k], err_msg=f"{k}: clean rows beside the stress rows")


def test_enrich_other_parameters_and_column_subset(cuda):
    """The generic (not unrolled) instantiation: windows 5 / 30 / 126,
    bb_ddof 0 and the other parameters of
    test_enrich_gpu.test_subset_of_columns_and_params, every column held to
    the exact value under the same parameters; the column subset of that test
    gives the same bits as the full launch."""
    s = sb.sides("other")
    p = engine.IndicatorParams(**sb.OTHER_PARAMS)
    assert p.as_oracle_dict() == {**ref.DEFAULTS, **sb.OTHER_PARAMS}
    got = _enrich(s.panel, params=p)
    _check_enrich(s, got, COLS, "enrich-other")
    _check_plateaus(s, got, COLS, sb.OTHER_PARAMS["ma_periods"], sb.OTHER_PARAMS["bb_window"])
    sub = _enrich(s.panel, params=p, columns=sb.OTHER_COLUMNS)
    assert set(sub) == set(sb.OTHER_COLUMNS)
    for k in sb.OTHER_COLUMNS:
        np.testing.assert_array_equal(sub[k], got[k], err_msg=f"{k}: column subset")


@pytest.mark.parametrize("frame", [0, 128])
@pytest.mark.parametrize("span", [(1000, 1100), (2000, 2100)])
def test_tick_path(cuda, frame, span):
    """engine.TickState seeded with [0, T0) and ticked through [T0, T1): the
    /10 and /100 candles at 1024, the plateau across the tile edge and the
    events at 2048 pass through the ring. Window columns: the rule above
    against the exact values and pandas over [0, t] (frame 0) or over the
    frame [t - 127, t] (frame 128, pandas through tick_frame_rows); pandas is
    consulted only where the kernel is outside the bar, and only on the pairs
    the CPU test lists. The EMA family bit-equal to pandas' ewm over the
    frame."""
    s = sb.sides("default")
    T0, T1 = span
    P = s.panel
    d = _dev(P)
    st = engine.TickState(len(s.names), frame=frame)
    st.seed(*(d[k][:, :T0] for k in FIELDS))
    window_cols = [k for k in COLS if k not in sb.EMA_FAMILY]
    worst = {k: np.zeros(len(s.names)) for k in window_cols}
    waived = set()
    for t in range(T0, T1):
        out = st.tick([d[k][:, t].contiguous() for k in FIELDS])
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
        if frame:
            a = t - frame + 1
            exact = {k: v[:, -1] for k, v in
                     exact_ref.enrich(*(P[k][:, a : t + 1] for k in FIELDS), with_ema=False).items()}
            ema = ref.ema_family_frame(P["close"], t, frame)
        else:
            exact = {k: s.exact[k][:, t] for k in window_cols}
            ema = {k: s.pandas[k][:, t] for k in sb.EMA_FAMILY}
        for k in sb.EMA_FAMILY:
            np.testing.assert_array_equal(out[k], ema[k], err_msg=f"{k}@{t}")
        pandas_t = None
        for k in window_cols:
            sc = s.scale[k] if np.isscalar(s.scale[k]) else s.scale[k][:, t]
            sb.assert_nan_pattern(out[k], np.asarray(exact[k], dtype=np.float64), f"{k}@{t}")   # = pandas' (CPU test)
            off = sb.outside(out[k], exact[k], sc)
            worst[k] = np.maximum(worst[k], np.nan_to_num(sb.ratio(out[k], exact[k], sc)))
            if not off.any():
                continue
            if pandas_t is None:
                pandas_t = (ref.tick_frame_rows(*(P[f] for f in FIELDS), t, frame) if frame
                            else {c: s.pandas[c][:, t] for c in COLS})
            sb.assert_held(out[k], exact[k], pandas_t[k], sc, f"{k}@{t}", s.names)
            waived |= {(s.names[i], k) for i in np.flatnonzero(off)}
    assert st.count == T1
    assert waived <= set(sb.PANDAS_OUTSIDE["default"]), f"outside the bar on unlisted pairs: {sorted(waived)}"
    _report(f"tick frame={frame} [{T0},{T1})", s.names, worst)


def _signal_forms(panel):
    from binquant_amd import signals

    d = _dev(panel)
    h, l, c = d["high"], d["low"], d["close"]
    out = {
        "wilder_rsi": (signals.wilder_rsi(c), signals.wilder_rsi(c, exact=True)),
        "adx": (signals.adx(h, l, c), signals.adx(h, l, c, exact=True)),
        "zscore": (signals.zscore(c), signals.zscore(c, exact=True)),
    }
    torch.cuda.synchronize()
    return {k: (a.cpu().numpy(), b.cpu().numpy()) for k, (a, b) in out.items()}


@pytest.mark.parametrize("kind", ["default", "long"])
def test_signal_helpers(cuda, kind):
    """signals.wilder_rsi / adx / zscore, the time-parallel form and
    exact=True, on the 17 families and on T = 4100 rows whose crash and
    plateau lie on candle 2048 (the carry of these kernels' tiles). On the
    ramps both forms give the same side of the RSI 30 / 70 and ADX 25 cuts at
    every candle where the exact value is further than its bar from the cut."""
    s = sb.sides(kind)
    sides = s.signal_sides()
    forms = _signal_forms(s.panel)
    worst = {}
    for k, (ex, pdv) in sides.items():
        for form, got in zip(("fast", "replay"), forms[k]):
            r = sb.assert_held(got, ex, pdv, s.scale[k], f"{kind}.{k}.{form}", s.names)
            worst[f"{k}.{form}"] = np.nanmax(np.where(np.isnan(r), 0.0, r), axis=1)
    _report(f"signals {kind}", s.names, worst)
    if kind == "default":
        rows = [s.row("ramp_up"), s.row("ramp_down")]
        for k, cuts in (("wilder_rsi", (30.0, 70.0)), ("adx", (25.0,))):
            fast, replay = (x[rows] for x in forms[k])
            for cut in cuts:
                n = sb.assert_same_side(fast, replay, sides[k][0][rows], cut, 100.0, f"{k} cut {cut}")
                assert n >= 2 * (2300 - 40), f"{k} cut {cut}: only {n} candles compared"


def test_market_features(cuda):
    """engine.market_features(max_bars=400) against
    market_ref.panel_features_at by test_market_gpu's rule (1e-9 relative,
    scale 1e-3). Where that fails, the long-double restatement of the feature
    decides: it must be within the rule of the kernel, and pandas further from
    it than the kernel — allowed only in the pairs where pandas itself is
    outside the rule around the restatement, which test_stress_ref pins:
    bb_width (a rolling std, ddof 0) after the /10 and /100 crashes and in the
    pump-and-dump row. (The issue expected ramp_down and the /100 crash from
    the enrich measurement; under the 400-bar cap the ramp's frame has fallen
    by e^-2 only and pandas is inside the rule there, while after a /10 candle
    it is 5e-9 off: FEATURE_PANDAS_OUTSIDE, measured on the CPU.)"""
    s = sb.sides("default")
    d = _dev(s.panel)
    f = engine.market_features(d["high"], d["low"], d["close"], max_bars=400)
    torch.cuda.synchronize()
    f = {k: v.cpu().numpy() for k, v in f.items()}
    H, L, C = (s.panel[k] for k in ("high", "low", "close"))
    arbitrated = {}
    worst = {k: np.zeros(len(s.names)) for k in FEATURE_COLUMNS}
    assert sb.FEATURES == FEATURE_COLUMNS
    candles = sb.feature_candles(s)
    assert len(candles) > 300
    for i, t in candles:
        want = market_ref.panel_features_at(H[i], L[i], C[i], t, 400)
        exact = None
        for k in FEATURE_COLUMNS:
            g, w = float(f[k][i, t]), float(want[k])
            assert np.isfinite(g), (k, s.names[i], t)
            if sb.feature_rule(g, w):
                continue
            if exact is None:
                exact = sb.features_exact(H[i], L[i], C[i], t)
            e = exact[k]
            assert sb.feature_rule(g, e), f"{k}[{s.names[i]},{t}]: got {g!r}, exact {e!r}, pandas {w!r}"
            assert abs(w - e) > abs(g - e), f"{k}[{s.names[i]},{t}]: pandas {w!r} is closer to {e!r} than {g!r}"
            arbitrated.setdefault((s.names[i], k), []).append(t)
        if exact is None:
            exact = sb.features_exact(H[i], L[i], C[i], t)
        for k in FEATURE_COLUMNS:
            lim = 1e-9 * abs(exact[k]) + 1e-14
            worst[k][i] = max(worst[k][i], abs(float(f[k][i, t]) - exact[k]) / lim)
    print("stress: market_features arbitrated", {k: len(v) for k, v in arbitrated.items()})
    _report("market_features", s.names, worst)
    assert set(arbitrated) <= set(sb.FEATURE_PANDAS_OUTSIDE), arbitrated
