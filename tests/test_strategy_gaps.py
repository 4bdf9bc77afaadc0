"""tests/golden/strategy_gaps.npz without a device: the fixture loads, the
regenerated panel matches its digest, every case holds the missing values its
description names (tests/golden/strategy_gaps_panel_gen.py) and nothing else,
and the reference's detectors fire after the gaps — so the GPU parity test
(tests/test_strategy_gaps_gpu.py) compares live signals, not rows of zeros."""

import numpy as np
import pytest

from tests import strategy_gaps as sg

gen = sg.gen
ALL = ("open", "high", "low", "close", "volume")
OHLC = ("open", "high", "low", "close")
T = gen.T_SHORT


def _r(a, b):
    return list(range(a, b + 1))


# case -> {field: candles that are NaN}; written out here, not read from the generator
LAYOUT = {
    "one_nan_close": {"close": [100]},
    "candle_run": {f: _r(75, 79) for f in ALL},
    "late_listing": {f: _r(0, 59) for f in ALL},
    "nan_volume": {"volume": [60, 61, 105]},
    "nan_tail": {f: [198, 199] for f in ALL},
    "empty_bins": {f: [50, 51, 52, 115] for f in OHLC},
    "nan_at_zero": {f: [0] for f in ALL},
    "nan_open": {"open": [90, 91]},
    "close_w_burst": {"close": [T - 1 - 82]},
    "close_w_pump": {"close": [T - 1 - 50]},
    "close_w_spike": {"close": [T - 1 - 60]},
    "close_run_lags": {"close": _r(100, 105)},
    "nan_after_spike": {f: [111] for f in ALL},
    "bench_overlap": {f: [90, 91, 92, 93, 111] for f in ALL},
    "clean_a": {},
    "clean_b": {},
    "long_close_1023": {"close": [1023]},
    "long_run_1020": {f: _r(1020, 1030) for f in ALL},
    "long_listing_1024": {f: _r(0, 1023) for f in ALL},
    "long_run_halo": {f: _r(985, 1030) for f in ALL},
}
# detectors that cannot fire after the row's last gap (make_golden_strategy_gaps.py states why)
NO_FIRE = {"nan_tail": ("qualified_signal", "score_cross", "label"), "close_w_pump": ("score_cross",),
           "scattered_nan_high": ("score_cross",), "long_run_1020": ("score_cross",),
           "long_run_halo": ("score_cross",)}


@pytest.fixture(scope="module")
def z():
    return sg.load()


def test_fixture_loads_and_panel_matches_digest(z):
    P = sg.panels()   # asserts the digest and the stored inputs
    assert [str(c) for c in z["cases"]] == list(gen.SHORT_CASES + gen.LONG_CASES)
    assert P["short"]["close"].shape == (17, 200) and P["long"]["close"].shape == (4, 1100)
    for tag, (cases, Tt, lo, _) in sg.TAGS.items():
        sg.bench_aligned(tag)
        for prefix in ("abp", "lsp", "fsf"):
            for k in sg.columns(prefix):
                a = z[f"{tag}__{prefix}__{k}"]
                assert a.shape == (len(cases), Tt - lo), (tag, prefix, k)
                assert a.dtype in (np.float64, np.uint8), (tag, prefix, k, a.dtype)
        pos = z[f"{tag}__a20_positions"]
        assert pos.max() == Tt - 1 and ((pos >= lo) | (pos == -1)).all()
    for k in ("qualified_signal", "vol_spike"):
        assert z[f"short__abp__{k}"].dtype == np.uint8
    for k in ("label", "suppressed_label", "label_pre", "upward", "vol_compression_flag"):
        assert z[f"short__fsf__{k}"].dtype == np.uint8
    assert z["short__lsp__score_cross"].dtype == np.uint8
    # per-row price scales over 1e-2 .. 1e3
    first = np.array([row[np.isfinite(row)][0] for row in P["short"]["close"]])
    assert first.min() < 2e-2 and first.max() > 5e2


@pytest.mark.parametrize("tag,i,case", sg.CASES, ids=[c for _, _, c in sg.CASES])
def test_nan_layout(z, tag, i, case):
    P = sg.panels()[tag]
    if case == "scattered_nan_high":
        for f in ("open", "low", "close", "volume"):
            assert not np.isnan(P[f][i]).any(), f
        ts = np.flatnonzero(np.isnan(P["high"][i]))
        assert len(ts) >= 5 and (np.diff(ts) < 48).all() and (np.diff(ts) > 1).all()
        assert ts[0] < 48 and ts[-1] > T - 48   # the pump's 48-bar threshold never sees a clean window
        return
    want = LAYOUT[case]
    for f in ALL:
        np.testing.assert_array_equal(np.flatnonzero(np.isnan(P[f][i])), want.get(f, []), err_msg=f"{case}.{f}")
    qv_nan = sorted(set(want.get("close", [])) | set(want.get("volume", [])))
    if case == "empty_bins":   # a resample's empty bin: no trades, volume and quote volume 0
        assert (P["volume"][i][[50, 51, 52, 115]] == 0.0).all()
        assert (P["quote_asset_volume"][i][[50, 51, 52, 115]] == 0.0).all()
        qv_nan = []
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(P["quote_asset_volume"][i])), qv_nan)
    assert gen.last_gap(case) == max([t for ts in want.values() for t in ts], default=-1)


def test_benchmark_gaps_meet_the_overlap_row(z):
    keep = z["short__bench_keep"]
    miss = set(np.flatnonzero(~keep))
    assert {88, 89, 90, 91, 110} <= miss       # 90, 91 inside the row's gap 90..93; 110 next to its gap at 111
    assert 111 not in miss and 92 not in miss
    assert (~z["long__bench_keep"][1019:1022]).all() and not z["long__bench_keep"][1031]


@pytest.mark.parametrize("tag,i,case", sg.CASES, ids=[c for _, _, c in sg.CASES])
def test_detectors_fire_after_the_gaps(z, tag, i, case):
    lo = sg.TAGS[tag][2]
    row = sg.TAGS[tag][3] + i
    after = max(gen.last_gap(case) + 1 - lo, 0)
    cols = {"qualified_signal": "abp__qualified_signal", "score_cross": "lsp__score_cross", "label": "fsf__label",
            "suppressed_label": "fsf__suppressed_label"}
    for k, col in cols.items():
        n = int(z[f"{tag}__{col}"][i, after:].sum())
        assert n == int(z[f"fire__{k}"][row]), (case, k)
        if k != "suppressed_label" and k not in NO_FIRE.get(case, ()):
            assert n > 0, f"{case}: {k} never fires after candle {gen.last_gap(case)}"


def test_suppressed_labels_and_the_scattered_high_row(z):
    assert int((z["fire__suppressed_label"] > 0).sum()) >= 3
    i = gen.SHORT_CASES.index("scattered_nan_high")
    assert int(z["short__lsp__score_cross"][i].sum()) == 0 == int(z["score_cross_scattered_sum"])
    assert np.isnan(z["short__lsp__score_threshold"][i]).all()
    # the windows of the three close_w_* rows are clean again exactly at the last candle
    j = gen.SHORT_CASES.index("close_w_pump")
    thr = z["short__lsp__score_threshold"][j]
    assert np.isnan(thr[T - 2]) and np.isfinite(thr[T - 1])
    j = gen.SHORT_CASES.index("close_w_burst")
    score = z["short__abp__activity_burst_score"][j]
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(score[20:])) + 20, [T - 83, T - 82])   # 20: the baseline's warm-up
    # the cooldown's state carries over a missing candle: the burst at 110 is labelled, the missing
    # candle 111 (a burst before it was blanked) is not, the burst at 115 is suppressed by 110's
    # 8-bar cooldown across the gap, the one at 119 is outside it
    j = gen.SHORT_CASES.index("nan_after_spike")
    pre, lab, sup = (z[f"short__fsf__{k}"][j] for k in ("label_pre", "label", "suppressed_label"))
    assert (pre[110], lab[110], pre[111], lab[111]) == (1, 1, 0, 0)
    assert (pre[115], lab[115], sup[115]) == (1, 0, 1) and (lab[119], sup[119]) == (1, 0)
    # pandas' own drift in the five std columns: under half of tests/spike_std.py's cap
    for name, (n_bad, n) in zip(z["std_drift_columns"], z["std_drift_cells"]):
        assert n_bad < 0.005 * n, (str(name), int(n_bad), int(n))
    assert len(z["std_drift_columns"]) == 5


def test_recorded_pandas_version(z):
    import pandas as pd

    if str(z["pandas_version"]) != pd.__version__:
        pytest.skip(f"strategy_gaps.npz was recorded with pandas {z['pandas_version']}, installed {pd.__version__}: "
                    "regenerate it (tests/golden/make_golden_strategy_gaps.py)")
