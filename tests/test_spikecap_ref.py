"""The numpy restatement of FailedSpikeFade.latest_signal() under a sliding
frame cap (tests/spikecap_ref.py) against what a FRESH instance of the real
class returned on every capped frame df.iloc[max(first, t + 1 - M):t + 1]
(tests/golden/spikecap.npz, M = 64, 96, 301). The slow form (one cut-out
frame per cell through tests/spikeframes_ref's functions) is the oracle of
the device tests: booleans exact, thresholds bit-equal to the recording. The
fast form restates the kernels' frame-local rules on one set of row columns:
booleans exact, thresholds to 1e-9 relative of the slow form."""

import numpy as np
import pytest

from tests import spikecap_cases as sc
from tests.spikecap_cases import cref, pg, ref

CAPS = pg.CAPS
DIFF = ("label", "price_break_flag", "cumulative_price_break_flag")


def coverage():
    return {k: int(v) for k, v in (x.split("=") for x in sc.fixture()["coverage"])}


def total(cov, key):
    return sum(v for k, v in cov.items() if k.endswith(key))


def test_fixture_covers_what_it_is_for():
    """The stored coverage line: (a) cells that differ from the expanding-frame
    answer, (b) walks that start inside a slid frame's first 60 rows, (c) cells
    where the shortcut's label is wrong, (d) frames that start on a missing
    close and move the price floor, (e) no near-tie."""
    fx, cov = sc.fixture(), coverage()
    assert tuple(fx["caps"]) == CAPS == (64, 96, 301)
    assert cov["c64_differs"] >= 20 and cov["c301_differs"] >= 1
    assert total(cov, "_zone_walks") >= 20
    assert total(cov, "_shortcut_label_wrong") >= 3
    assert total(cov, "_missing_start") >= 5 and total(cov, "_missing_start_floor_moved") >= 1
    assert cov["ties"] == 0
    assert (fx["in_frame"] == sc.in_frame(sc.panel())).all() and cov["cells"] == fx["in_frame"].sum()
    p = sc.panel()
    assert p["close"].shape == (8, 420) and (p["first_t"] > 0).sum() == 2 and (p["lens"] < 420).sum() == 1


@pytest.mark.parametrize("cap", CAPS)
def test_slow_restatement_equals_fresh_instances(cap):
    fx, mask = sc.recorded(cap), sc.in_frame(sc.panel())
    got, _ = sc.ref_fixture(cap)
    sc.assert_bools_equal(got, fx, mask, f"cap {cap}")
    for k in sc.THRESHOLDS:
        assert sc.same_bits(got[k][mask], fx[k][mask]).all(), k
    sc.assert_fill(got, mask, f"cap {cap}")


@pytest.mark.parametrize("cap", CAPS)
def test_fast_restatement_equals_slow_and_counts_the_coverage(cap):
    """The kernels' rules on the row's columns give the cut-out frames' answer;
    the counts the generator stored, on the restatement's own output."""
    mask, cov = sc.in_frame(sc.panel()), coverage()
    slow, _ = sc.ref_fixture(cap)
    fast, zone = sc.ref_fixture(cap, fast=True)
    sc.assert_matches(fast, slow, mask, f"fast, cap {cap}")
    expanding, _ = sc.ref_fixture(None)
    differs = np.zeros_like(mask)
    for k in DIFF:
        differs |= (slow[k] != expanding[k]) & mask
    assert differs.sum() == cov[f"c{cap}_differs"]
    short, _ = sc.ref_fixture(cap, fast=True, shortcut=True)
    wrong = (short["label"] != slow["label"]) & mask
    assert wrong.sum() == cov[f"c{cap}_shortcut_label_wrong"]
    assert (sc.recorded(cap)["label"][wrong] == slow["label"][wrong]).all()   # the recording is right there
    if cap == 64:
        assert differs.sum() >= 20 and wrong.sum() >= 3 and len(zone) >= 20
    for k in sc.THRESHOLDS:   # the shortcut's thresholds are the sliding ones
        assert (np.abs(short[k] - slow[k])[mask] <= sc.RTOL * np.abs(slow[k][mask])).all()


def test_frame_that_starts_on_a_missing_close_loses_the_run():
    """(d): with the close missing on a slid frame's first row, the rows up to
    the first valid close have a finite change in the row's columns (0.0 from
    the pad fill, then the jump) and none in the frame: the recorded price
    floor is not the quantile of the row's own finite changes inside it."""
    p, fx = sc.panel(), sc.recorded(64)
    cells = moved = 0
    for s in range(pg.S):
        a, b = int(p["first_t"][s]), int(p["lens"][s])
        pca = ref.frame_columns(p["open"][s, a:b], p["close"][s, a:b], p["volume"][s, a:b], ref.Params())[
            "price_change_abs"]
        for t in range(a + 64, b):
            f = t + 1 - 64
            if np.isnan(p["close"][s, f]):
                x = pca[f + 1 - a:t + 1 - a]
                naive = max(0.03, 0.015, float(np.quantile(x[~np.isnan(x)], 0.75)))
                cells += 1
                moved += int(naive != fx["price_break_base_threshold"][s, t])
    cov = coverage()
    assert cells == cov["c64_missing_start"] >= 5 and moved == cov["c64_missing_start_floor_moved"] >= 1


def test_one_cell_of_a_frame_is_frames_rows_last():
    """frame_last (what the oracle runs per cut-out frame) against
    spikeframes_ref.frames_row on the same slice, on sampled cells."""
    p = sc.panel()
    labels = 0
    for s, t, cap in ((0, 100, 64), (3, 200, 64), (5, 150, 96), (6, 380, 301), (2, 419, 64), (1, 101, 64)):
        f = max(int(p["first_t"][s]), t + 1 - cap)
        sl = tuple(p[k][s, f:t + 1] for k in ("open", "close", "volume"))
        one, row = cref.frame_last(*sl, ref.Params()), ref.frames_row(*sl)
        for k in ref.KEYS:
            a, b = np.float64(one[k]), np.float64(row[k][-1])
            assert sc.same_bits(a, b).all(), (k, s, t)
        labels += int(one["label_pre"])
    assert labels >= 1


def test_cap_at_least_the_row_is_the_expanding_answer():
    p = sc.synth_panel(3, 90, seed=5)
    want = ref.frames(p["open"], p["close"], p["volume"])
    for cap in (90, 91, 2048):
        got = cref.frames(p["open"], p["close"], p["volume"], cap)
        for k in ref.KEYS:
            assert sc.same_bits(got[k], want[k]).all() if got[k].dtype == np.float64 else (got[k] == want[k]).all()
