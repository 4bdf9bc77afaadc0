"""CPU: the numpy restatement (tests/rsreversal_ref.py) equals what the real
RelativeStrengthReversalRange.signal() did (tests/golden/rsreversal_gates.npz,
recorded by tests/golden/make_golden_rsreversal.py): codes exact, the floor
equal or both NaN. Its quantile is pd.Series.quantile bit for bit, and is not
pandas' rolling quantile."""

import numpy as np
import pandas as pd
import pytest

from tests import rsreversal_cases as rc
from tests.rsreversal_cases import pg, ref

W, Q = ref.DEFAULTS["window"], ref.DEFAULTS["quantile"]


def test_fixture_is_what_it_is_for():
    fx, p, rec = rc.fixture(), rc.panel(), rc.recorded()
    assert list(fx["default_names"]) == list(ref.DEFAULTS)
    assert fx["defaults"].tolist() == [float(v) for v in ref.DEFAULTS.values()]
    assert tuple(fx["reasons"]) == ref.REASONS and tuple(fx["names"]) == pg.NAMES
    status, floor, vol = rec["status"], rec["volume_floor"], p["volume"]
    assert status.shape == (pg.S, pg.T) == vol.shape
    counts = np.bincount(status.ravel(), minlength=10)
    assert len(counts) == 10 and (counts >= 20).all(), counts
    assert (p["first_t"] > 0).sum() >= 3 and (p["lens"] < pg.T).sum() >= 3
    reached = (status == ref.EMIT) | (status == ref.DEAD_TAPE)
    emit = status == ref.EMIT
    assert np.isnan(floor[~reached]).all()
    parts = {(s, t): ref.quantile_parts(vol[s, t - W + 1:t + 1], Q) for s, t in np.argwhere(reached)}
    assert sum(n < W for n, *_ in parts.values()) >= 20
    assert sum(g >= 0.5 for _, g, *_ in parts.values()) >= 3 and sum(0 < g < 0.5 for _, g, *_ in parts.values()) >= 3
    # a finite rank beside an infinite one: a NaN floor, and the message went out
    beside = [k for k, (n, g, a, b) in parts.items() if n and np.isinf(a) != np.isinf(b)]
    assert len(beside) >= 3 and all(np.isnan(floor[k]) for k in beside) and sum(emit[k] for k in beside) >= 3
    ties = reached & (vol == floor)
    assert ties.sum() >= 3 and (status[ties] == ref.DEAD_TAPE).all()
    assert (np.isnan(vol) & emit).sum() >= 3
    with np.errstate(invalid="ignore"):
        near = reached & ~ties & np.isfinite(floor) & np.isfinite(vol) & (np.abs(vol - floor) < 1e-9 * np.abs(floor))
    assert near.sum() == 0
    assert sum(np.isnan(vol[s, t - W + 1:t + 1]).all() for s, t in parts) >= 1   # no observation: NaN, emitted
    t = np.arange(pg.T)[None, :]
    assert (reached & ((t - W + 1) // 64 != t // 64)).sum() >= 3
    # the gates let a NaN through and refuse the limit itself
    assert (np.isnan(p["average_return"])[None, :] & reached).any() and (np.isnan(p["rs"]) & reached).any()
    assert ((p["average_return"] == pg.AVG_RETURN_MAX)[None, :] & (status == ref.MARKET_NOT_WEAK)).any()
    assert ((p["rs"] == pg.RS_MIN) & (status == ref.RS_INSUFFICIENT)).any()
    # a whole 64-candle step past the frame gate with no reaching candle beside one that has some
    quiet = [(s, k) for s in range(pg.S) for k in (1, 2)
             if (status[s, 64 * k:64 * k + 64] >= ref.NO_CONTEXT).all() and not reached[s, 64 * k:64 * k + 64].any()
             and (reached[s, 64 * k - 64:64 * k].any() or reached[s, 64 * k + 64:64 * k + 128].any())]
    assert len(quiet) >= 1


def test_replay_equals_the_recording():
    got, want = rc.fixture_replay(), rc.recorded()
    rc.assert_codes_equal(got, want, "restatement")
    rc.assert_values_equal(got, want, "restatement")


def test_rolling_quantile_is_not_the_method():
    """The staged form's floor (pandas' rolling quantile of the same window)
    differs from the recording at 20 cells or more, and changes decisions."""
    want, staged = rc.recorded(), rc.fixture_replay(rolling=True)
    reached = (want["status"] == ref.EMIT) | (want["status"] == ref.DEAD_TAPE)
    differs = reached & ~rc.same_value(want["volume_floor"], staged["volume_floor"])
    assert differs.sum() >= 20
    assert (staged["status"] != want["status"]).sum() >= 3
    with pytest.raises(AssertionError):
        rc.assert_values_equal(staged, want)


def random_windows(n=4000, seed=7):
    """Windows of 1-192 values with duplicates, NaN, +-inf and zeros."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        m = int(rng.integers(1, 193))
        w = np.round(rng.lognormal(1.0, 1.0, m), int(rng.integers(0, 3)))
        for value, share in ((np.nan, rng.choice([0.0, 0.05, 0.5, 1.0], p=[0.3, 0.4, 0.2, 0.1])),
                             (np.inf, rng.choice([0.0, 0.03, 0.8], p=[0.5, 0.3, 0.2])),
                             (-np.inf, rng.choice([0.0, 0.03], p=[0.8, 0.2])), (0.0, rng.choice([0.0, 0.2]))):
            w[rng.random(m) < share] = value
        yield w, float(rng.choice([0.0, 0.2, 0.5, 0.92, 1.0, rng.random()]))


def test_series_quantile_is_pandas_bit_for_bit():
    rolled = 0
    with np.errstate(invalid="ignore"):
        for w, q in random_windows():
            want, got = pd.Series(w).quantile(q), ref.series_quantile(w, q)
            assert (np.isnan(want) and np.isnan(got)) or np.float64(want).view(np.int64) == np.float64(got).view(np.int64), \
                (w.tolist(), q, want, got)
            r = pd.Series(w).rolling(len(w), min_periods=1).quantile(q).iloc[-1]
            mine = ref.rolling_quantile(w, q)
            assert (np.isnan(r) and np.isnan(mine)) or r == mine, (w.tolist(), q, r, mine)
            rolled += not ((np.isnan(r) and np.isnan(want)) or r == want)
    assert rolled >= 200   # the rolling quantile of the same window is another number on many of them


def test_quantile_by_hand():
    inf, nan = float("inf"), float("nan")
    assert ref.series_quantile([1.0, 2.0, 3.0, 4.0, 5.0], 0.5) == 3.0
    assert ref.series_quantile([5.0, nan, 1.0], 0.2) == 1.0 + 4.0 * 0.2
    assert np.isnan(ref.series_quantile([nan, nan], 0.2)) and np.isnan(ref.series_quantile([], 0.2))
    # the lerp is applied at a zero fraction too: finite + inf * 0
    assert np.isnan(ref.series_quantile([1.0, inf], 0.0)) and ref.rolling_quantile([1.0, inf], 0.0) == 1.0
    assert np.isnan(ref.series_quantile([inf], 0.2)) and np.isnan(ref.rolling_quantile([inf], 0.2))
    w = [1.0] * 20 + [inf] * 76   # n = 96: s[19] finite, s[20] infinite
    assert np.isnan(ref.series_quantile(w, 0.2)) and ref.rolling_quantile(w, 0.2) == 1.0
    assert ref.series_quantile([0.1, 0.2, 0.4], 0.92) == 0.4 - (0.4 - 0.2) * (1.0 - (2 * 0.92 - 1.0))


def test_split_frames_equal_the_whole():
    """The method keeps no state: a replay split through lens / from_t equals the whole."""
    p, whole = rc.panel(), rc.fixture_replay()
    rows = slice(0, 8)
    q = dict(volume=p["volume"][rows], context_ok=p["context_ok"], market_regime=p["market_regime"],
             average_return=p["average_return"], features_ok=p["features_ok"][rows], rs=p["rs"][rows])
    for k in (127, 128, 129):
        a = rc.ref_replay(q, first_t=p["first_t"][rows], lens=np.minimum(p["lens"][rows], k))
        b = rc.ref_replay(q, first_t=p["first_t"][rows], lens=p["lens"][rows], from_t=np.full(8, k))
        for name in ("status",) + ref.VALUES:
            joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
            assert rc.same_value(joined, whole[name][rows]).all(), (k, name)
