"""CPU: the two references of the stress rows against each other.

tests/test_stress_gpu.py holds the kernels to
err(kernel) <= max(bar, err(pandas)) around the long-double values of
tests/exact_ref.py (bar and scales: tests/stress_bar.py). That comparison is
only as good as the exact reference, and only as tight as pandas' own error
lets it be; both are pinned here, at the shapes the GPU tests use, so that a
broken reference or a changed family cannot quietly waive it.

Where pandas leaves the bar (worst err(pandas) / bar, share of the row's
candles outside; pandas 2.3.3, T = 2300; nowhere else, on no column):

  default parameters (bb_window 20, ddof 1)
    ramp_down      bb_upper 4.2e4   46 %    bb_lower 4.7e4   47 %
    crash100@1024  bb_upper 28      55 %    bb_lower 29      55 %
  OTHER_PARAMS (bb_window 10, ddof 0, k 2.5)
    ramp_down      bb_upper 4.3e5   56 %    bb_lower 4.6e5   57 %
    crash100@1024  bb_upper 145     55 %    bb_lower 145     55 %
    crash10@1024   bb_upper 1.3     0.4 %   bb_lower 1.3     0.4 %
  z-score(20) (the rolling std at ddof 0; bar 1e-9 |z| + 1e-11)
    ramp_down 7.7e5  59 %    crash100@1024 1.0e4  55 %   crash10@1024 109  55 %
    crash10@700 74   69 %    pump_dump 24         60 %
  Wilder RSI, ADX, and every column of the T = 4100 rows: none.

All of it is pandas' online rolling variance: after a /10 or /100 candle, and
along a ramp that has fallen by e^-11, its running sum of squares still
carries the rounding of the large prices that left the window. The ramp's
ratios are larger than a T = 1300 ramp's (21x) because the row falls further.
pandas' rolling means and sums (Kahan-compensated) stay within 3e-7 of the
bar on every family, its NaN pattern equals the exact one everywhere.
"""

import numpy as np
import pytest

from tests import exact_ref, stress_bar as sb, stress_cases

PANDAS_OUTSIDE = sb.PANDAS_OUTSIDE


def quantities(s: sb.Sides, signals: bool) -> dict:
    q = {k: (s.exact[k], s.pandas[k], s.scale[k]) for k in exact_ref.CANONICAL}
    if signals:
        q.update({k: (e, p, s.scale[k]) for k, (e, p) in s.signal_sides().items()})
    return q


def test_rows_are_what_the_issue_describes():
    fams = stress_cases.families()
    assert stress_cases.names(fams) == [
        "ramp_up", "ramp_down", "tick2_plateau", "crash10@700", "crash10@1024", "crash10@2048", "spike10@700",
        "spike10@1024", "spike10@2048", "crash100@1024", "spike100@1024", "pump_dump", "micro", "huge", "zigzag",
        "tight_high", "vol_drop_1e4"]
    by = {f.name: f for f in fams}
    for f in fams:
        for k in stress_cases.FIELDS:
            x = getattr(f, k)
            assert x.shape == (2300,) and np.isfinite(x).all(), (f.name, k)
        assert (f.high >= np.maximum(f.open, f.close)).all() and (f.low <= np.minimum(f.open, f.close)).all(), f.name
        assert (f.open[1:] == f.close[:-1]).all() and (f.low > 0).all() and (f.volume >= 0).all(), f.name
        flat = np.r_[False, f.close[1:] == f.close[:-1]]
        assert (f.high[flat] == f.low[flat]).all() and (f.high[~flat][1:] > f.low[~flat][1:]).all(), f.name
    assert np.allclose(np.diff(np.log(by["ramp_up"].close)), 0.005, atol=1e-12)
    assert np.allclose(np.diff(np.log(by["ramp_down"].close)), -0.005, atol=1e-12)
    for name, e, fac in (("crash10@700", 700, 0.1), ("crash10@1024", 1024, 0.1), ("crash10@2048", 2048, 0.1),
                         ("spike10@700", 700, 10), ("spike10@1024", 1024, 10), ("spike10@2048", 2048, 10),
                         ("crash100@1024", 1024, 0.01), ("spike100@1024", 1024, 100)):
        c = by[name].close
        assert by[name].events == (e,)
        assert abs(c[e] / c[e - 1] / fac - 1) < 0.01 and np.abs(np.delete(np.diff(np.log(c)), e - 1)).max() < 0.01
    t2 = by["tick2_plateau"]
    assert t2.plateaus == ((200, 240), (1010, 1130), (2040, 2060)) and t2.zero_volume == ((300, 330), (1015, 1045))
    assert (t2.close == np.round(t2.close, 2)).all() and t2.close.min() >= 0.05 and (t2.volume == np.floor(t2.volume)).all()
    for a, b in t2.plateaus:
        assert (t2.close[a:b] == t2.close[a]).all() and t2.close[a - 1] != t2.close[a] != t2.close[b]
    for f in (t2, by["vol_drop_1e4"]):
        for a, b in f.zero_volume:
            assert (f.volume[a:b] == 0).all() and f.volume[a - 1] > 0 and f.volume[b] > 0
    vd = by["vol_drop_1e4"].volume
    assert 3e3 < np.median(vd[:600]) / np.median(vd[600:]) < 3e4
    pd_ = by["pump_dump"]
    r = np.diff(np.log(pd_.close))
    assert pd_.close[0] < 0.011 and np.isclose(r[149:159], np.log(1.35)).all() and np.isclose(r[159:165], np.log(0.6)).all()
    assert set(np.unique(by["zigzag"].close)) == {100.0, 100.01} and (np.diff(by["zigzag"].close) != 0).all()
    assert 2e9 < by["huge"].close.mean() < 5e9 and np.median(by["huge"].volume) > 1e10
    assert 5e-6 < by["micro"].close.mean() < 5e-5 and (by["micro"].close == np.round(by["micro"].close, 8)).all()
    th = by["tight_high"].close
    assert (th == np.round(th, 1)).all() and abs(th.mean() - 60000) < 0.1 and 0.4 < th.std() < 0.6
    lf = stress_cases.long_families()
    assert [f.name for f in lf] == ["crash10@2048", "tick2_plateau"] and all(f.close.size == 4100 for f in lf)
    assert (2040, 2060) in lf[1].plateaus and lf[0].events == (2048,)


@pytest.mark.parametrize("kind", ["default", "other", "long"])
def test_pandas_against_exact(kind):
    """pandas' NaN pattern is the exact one on every family and column; pandas
    is inside the bar at every candle of every (family, column) pair that is
    not listed above, and the listed pairs are the ones that are outside."""
    s = sb.sides(kind)
    q = quantities(s, signals=kind != "other")
    for k, (ex, pdv, _) in q.items():
        sb.assert_nan_pattern(pdv, np.asarray(ex, dtype=np.float64), f"{kind}.{k}")
    found = sb.pandas_outside_pairs(s, q)
    print({k: (f"{r:.3g}", f"{sh:.3f}") for k, (r, sh) in found.items()})
    listed = PANDAS_OUTSIDE[kind]
    assert set(found) == set(listed), (
        f"pandas outside the bar on {sorted(set(found) - set(listed))}, inside on listed {sorted(set(listed) - set(found))}")
    for pair, (_, share) in found.items():
        assert share <= listed[pair], f"{pair}: {share:.3f} of the candles outside, listed {listed[pair]}"


def test_pandas_features_against_exact():
    """market_ref.panel_features_at (pandas over the 400-bar frame) against the
    long-double restatement at the candles test_stress_gpu checks, by
    test_market_gpu's rule: outside only in bb_width, in the windows that
    still hold the pre-crash price level's rounding — the 8 candles after the
    /10 and /100 windows have emptied of the old prices (5e-9 and 8e-7
    relative) and 2 candles of the pump-and-dump row at the cap edge (1e-9).
    ramp_down, which the issue expected here, is inside: at [398, 402] the
    frame still starts at the row's first candles."""
    from oracle import market_ref

    s = sb.sides("default")
    H, L, C = (s.panel[k] for k in ("high", "low", "close"))
    found = {}
    for i, t in sb.feature_candles(s):
        want = market_ref.panel_features_at(H[i], L[i], C[i], t, 400)
        exact = sb.features_exact(H[i], L[i], C[i], t)
        for k in sb.FEATURES:
            if not sb.feature_rule(float(want[k]), exact[k]):
                found[(s.names[i], k)] = found.get((s.names[i], k), 0) + 1
    assert found == sb.FEATURE_PANDAS_OUTSIDE


def _flat_run(close):
    """Number of consecutive equal closes ending at each candle."""
    run = np.ones(close.size, dtype=int)
    for t in range(1, close.size):
        run[t] = run[t - 1] + 1 if close[t] == close[t - 1] else 1
    return run


def test_special_values_are_exact_in_the_reference():
    s = sb.sides("default")
    rsi, mfi = s.exact["rsi"], s.exact["mfi"]
    t = np.arange(2300)
    up, dn = s.row("ramp_up"), s.row("ramp_down")
    assert np.isnan(rsi[[up, dn], :13]).all()
    assert (rsi[up, 13:] == 100).all() and (rsi[dn, 13:] == 0).all()
    assert (mfi[up, 13:] == 100).all() and (mfi[dn, 13:] == 0).all()
    for i, f in enumerate(s.fams):
        # rsi: NaN before the 14th candle and where the window's 14 deltas are all zero:
        # 15 equal closes (14 at candle 13, whose window starts with the missing delta)
        run = _flat_run(f.close)
        want = (t < 13) | (run >= 15) | ((t == 13) & (run >= 14))
        np.testing.assert_array_equal(np.isnan(rsi[i]), want, err_msg=f"rsi NaN pattern of {f.name}")
        # mfi: NaN where no candle of the window carries money flow: zero volume, or a
        # typical price equal to the previous one (a flat candle after a flat candle)
        tp = (f.high + f.low + f.close) / 3
        dead = np.r_[True, (tp[1:] == tp[:-1])] | (f.volume == 0)
        cnt = np.convolve(dead.astype(int), np.ones(14, dtype=int))[: f.close.size]
        np.testing.assert_array_equal(np.isnan(mfi[i]), (t < 13) | (cnt == 14), err_msg=f"mfi NaN pattern of {f.name}")
    v = s.fams[s.row("vol_drop_1e4")]
    zero = np.zeros(2300, dtype=bool)
    for a, b in v.zero_volume:
        zero[a + 13 : b] = True   # the windows that 14 zero-volume candles fill
    np.testing.assert_array_equal(np.isnan(mfi[s.row("vol_drop_1e4"), 13:]), zero[13:])
    p = s.row("tick2_plateau")
    for a, b in s.fams[p].plateaus:
        assert np.isnan(rsi[p, a + 14 : b]).all() and not np.isnan(rsi[p, a + 13]) and not np.isnan(rsi[p, b])
        price = s.fams[p].close[a]
        for k, w in (("ma_7", 7), ("ma_25", 25), ("ma_100", 100), ("bb_mid", 20), ("bb_upper", 20), ("bb_lower", 20)):
            if a + w - 1 < b:
                assert (s.exact[k][p, a + w - 1 : b] == price).all(), (k, a)
                np.testing.assert_array_equal(s.pandas[k][p, a + w - 1 : b], price, err_msg=f"pandas {k} on plateau {a}")
    for k in ("rsi", "mfi"):   # what the GPU test compares bit for bit
        np.testing.assert_array_equal(s.pandas[k][[up, dn]], np.asarray(s.exact[k][[up, dn]], dtype=np.float64))


def test_exact_reference_agrees_with_rational_arithmetic():
    """The long-double windows against exact rational arithmetic (oracle
    exact_std / exact_zscore) at the candles where pandas is furthest off."""
    from oracle import indicators_ref as ref

    s = sb.sides("default")
    z = s.signal_sides()["zscore"][0]
    for name, ts in (("ramp_down", (700, 1500, 2299)), ("crash100@1024", (1024, 1043, 1044, 1500, 2299)),
                     ("crash10@700", (719, 720)), ("tick2_plateau", (239, 240, 1130))):
        i = s.row(name)
        c = s.panel["close"][i]
        for t in ts:
            sd = ref.exact_std(c[t - 19 : t + 1], ddof=1)
            up = float(s.exact["bb_upper"][i, t])
            want = float(c[t - 19 : t + 1].astype(exact_ref.LD).sum() / 20) + 2.0 * sd
            assert abs(up - want) <= 4e-16 * abs(want), (name, t, up, want)
            zz = ref.exact_zscore(c[t - 19 : t + 1])
            assert abs(float(z[i, t]) - zz) <= 1e-14 * max(abs(zz), 1e-3), (name, t, float(z[i, t]), zz)


# ---- the assertions of the GPU tests bite ------------------------------------------

def test_held_assertion_bites():
    """assert_held on stand-in kernel outputs built from the exact and pandas
    arrays: the exact values and pandas' own pass; a value 2x the bar off after
    the crash, a ramp rsi of 99.999999, a moved NaN, and an error as large as
    pandas' on a pair where pandas is inside the bar all fail."""
    s = sb.sides("default")
    for k in exact_ref.CANONICAL:
        ex, pdv, sc = s.exact[k], s.pandas[k], s.scale[k]
        sb.assert_held(np.asarray(ex, dtype=np.float64), ex, pdv, sc, k, s.names)
        sb.assert_held(pdv, ex, pdv, sc, k, s.names)
    k, i = "bb_upper", s.row("crash10@1024")
    ex, pdv, sc = s.exact[k], s.pandas[k], s.scale[k]
    for t in (1030, 1043, 1100, 2299):
        bad = np.asarray(ex, dtype=np.float64).copy()
        bad[i, t] += 2 * float(sb.bar(ex, sc)[i, t])
        with pytest.raises(AssertionError, match="outside"):
            sb.assert_held(bad, ex, pdv, sc, k, s.names)
    # the local scale: long after the /100 candle a row-mean scale leaves macd (a
    # difference near zero, all absolute term) a bar more than 10x wider
    j, m = s.row("crash100@1024"), s.exact["macd"]
    assert float(sb.bar(m, s.scale["macd"])[j, 2299]) < 0.1 * (1e-9 * abs(float(m[j, 2299])) + 1e-11 * s.panel["close"][j].mean())
    # on a listed pair the kernel may be as far off as pandas, no further
    i = s.row("crash100@1024")
    t = int(np.nanargmax(sb.ratio(pdv[i], ex[i], sc[i])))
    far = pdv.copy()
    far[i, t] = float(ex[i, t]) + 1.5 * (pdv[i, t] - float(ex[i, t]))
    with pytest.raises(AssertionError, match="outside"):
        sb.assert_held(far, ex, pdv, sc, k, s.names)
    rsi = np.asarray(s.exact["rsi"], dtype=np.float64).copy()
    rsi[s.row("ramp_up"), 1500] = 99.999999
    with pytest.raises(AssertionError, match="outside"):
        sb.assert_held(rsi, s.exact["rsi"], s.pandas["rsi"], 100.0, "rsi", s.names)
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(rsi[s.row("ramp_up"), 13:], 100.0)
    mfi = s.pandas["mfi"].copy()
    mfi[s.row("vol_drop_1e4"), 313] = 50.0   # a NaN candle given a value
    with pytest.raises(AssertionError, match="NaN pattern"):
        sb.assert_held(mfi, s.exact["mfi"], s.pandas["mfi"], 100.0, "mfi", s.names)
    ma = s.pandas["ma_100"].copy()
    ma[s.row("huge"), 50] = 3e9              # a warm-up candle given a value
    with pytest.raises(AssertionError, match="NaN pattern"):
        sb.assert_held(ma, s.exact["ma_100"], s.pandas["ma_100"], s.scale["ma_100"], "ma_100", s.names)


def test_signal_assertions_bite():
    s = sb.sides("default")
    sig = s.signal_sides()
    for k, (ex, pdv) in sig.items():
        sb.assert_held(pdv, ex, pdv, s.scale[k], k, s.names)
        bad = np.asarray(ex, dtype=np.float64).copy()
        i, t = s.row("spike10@2048"), 2060
        bad[i, t] += 3 * float(sb.bar(ex, s.scale[k])[i, t])
        with pytest.raises(AssertionError, match="outside"):
            sb.assert_held(bad, ex, pdv, s.scale[k], k, s.names)
    ex = sig["wilder_rsi"][0]
    side = sb.cut_sides(ex, ex, 70.0, 100.0)
    assert side.sum() > 100   # the ramps are compared at nearly every candle
    flipped = np.asarray(ex, dtype=np.float64).copy()
    flipped[s.row("ramp_up"), 1000] = 69.0
    with pytest.raises(AssertionError):
        sb.assert_same_side(flipped, np.asarray(ex, dtype=np.float64), ex, 70.0, 100.0, "rsi 70")
