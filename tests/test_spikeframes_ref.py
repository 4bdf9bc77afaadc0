"""The numpy restatement of FailedSpikeFade.latest_signal() on every frame
(tests/spikeframes_ref.py) against what a FRESH instance of the real class
returned on each frame df.iloc[first:t + 1] (tests/golden/spikeframes.npz),
and against the last_spike fields the pending-spike fixture recorded
(tests/golden/spikefade_gates.npz). Booleans exact; the thresholds bit-equal:
they are numpy's own quantile arithmetic on pandas' own columns."""

import numpy as np
import pytest

from tests import spikeframes_cases as sc
from tests.spikeframes_cases import ref


def test_fixture_covers_what_it_is_for():
    fx = sc.fixture()
    cov = dict(x.split("=") for x in fx["coverage"])
    assert int(cov["suppressed"]) >= 50 and int(cov["walk_over_64"]) >= 10 and int(cov["walk_over_128"]) >= 3
    assert int(cov["raised_floor"]) >= 100 and int(cov["skipped_calibration"]) >= 10
    assert int(cov["volume_floor"]) >= 5 and int(cov["whole_row_differs"]) >= 20 and int(cov["ties"]) == 0
    assert (fx["in_frame"] == sc.in_frame(sc.panel())).all() and int(cov["cells"]) == fx["in_frame"].sum()


def test_restatement_equals_fresh_instances():
    fx, mask = sc.fixture(), sc.in_frame(sc.panel())
    got, _ = sc.ref_fixture()
    sc.assert_bools_equal(got, fx, mask, "prefix loop")
    for k in ref.FLOAT_KEYS:
        assert sc.same_bits(got[k][mask], fx[k][mask]).all(), k
    sc.assert_fill(got, mask, "prefix loop")
    # the counts the generator asserted, on the restatement's own output
    assert (got["label_pre"] & ~got["label"]).sum() >= 50
    assert (got["price_break_base_threshold"][mask] > 0.03).sum() >= 100
    assert (got["volume_cluster_min_ratio"][mask] == 1.15).sum() >= 5
    skipped = (got["volume_cluster_min_ratio"] == 1.6) & (got["price_break_base_threshold"] == 0.03) & mask
    assert skipped.sum() >= 10


def test_back_walk_equals_walk_from_frame_start():
    """The cooldown's verdict from the nearest clear run equals the walk from
    the frame's first row, on walks that cross one and two 64-candle blocks."""
    fx, mask = sc.fixture(), sc.in_frame(sc.panel())
    full, _ = sc.ref_fixture()
    back, walks = sc.ref_fixture(back_walk=True)
    for k in ("label", "label_short"):
        assert (full[k] == back[k]).all(), k
    assert (walks > 64).sum() >= 10 and (walks > 128).sum() >= 3
    # the recorded walks are to the run's first row (>= the restatement's, which stops at the same run)
    assert walks.max() == max(fx["walk"].max(), fx["walk_short"].max())
    assert ((fx["walk"] > 0) == (fx["label_pre"] & mask)).all()


def test_whole_row_pass_is_not_the_per_frame_answer():
    """What this entry replaces: the columns of one detect() over the whole
    row differ from the per-frame ones on the recorded cells (and agree on
    each row's last candle, whose frame is the whole row)."""
    fx, p = sc.fixture(), sc.panel()
    mask = sc.in_frame(p)
    differs = np.zeros_like(mask)
    for k in ("label", "price_break_flag", "cumulative_price_break_flag"):
        differs |= (fx[f"whole_{k}"] != fx[k]) & mask
        last = fx[k][np.arange(len(p["lens"])), p["lens"] - 1]
        assert (fx[f"whole_{k}"][np.arange(len(p["lens"])), p["lens"] - 1] == last).all(), k
    assert differs.sum() >= 20
    rows = np.arange(len(p["lens"]))
    assert sc.same_bits(fx["whole_volume_cluster_min_ratio"], fx["volume_cluster_min_ratio"][rows, p["lens"] - 1]).all()


def test_restatement_reproduces_recorded_last_spike_fields():
    """The pending-spike fixture reused one instance per row; its running price
    floor never bit there, so its recorded last_spike fields and source gate
    are a second yardstick: all 4569 cells."""
    fx, p = sc.fade_fixture(), sc.fade_panel()
    mask = sc.in_frame(p)
    assert mask.sum() == 4569
    got = sc.ref_fade()
    for k in sc.FADE_FIELDS:
        assert (got[k][mask] == fx[f"spike_{k}"][mask].astype(bool)).all(), k
    assert sc.same_bits(got["close_open_ratio"][mask], fx["spike_close_open_ratio"][mask]).all()
    ok, reason = ref.source_allows(got, float(fx["max_candle_return"]))
    assert (ok[mask] == fx["source_ok"][mask]).all() and (reason[mask] == fx["source_reason"][mask]).all()
    assert fx["source_ok"][mask].sum() >= 20


@pytest.mark.parametrize("mode", ["first", "all"])
def test_label_modes_against_pandas(mode):
    """The 'first' / 'all' cluster label modes of the restatement against a
    direct pandas evaluation of volume_cluster_flag (:350-360) on sampled frames."""
    import pandas as pd

    p = sc.panel()
    s = 1
    par = ref.Params(volume_cluster_label_mode=mode, volume_quantile=0.8)   # clusters are common below q97
    cols = ref.frame_columns(p["open"][s], p["close"][s], p["volume"][s], par)
    seen = 0
    for t in (40, 150, 287):
        vc, pb = ref.thresholds(cols, t, par)
        f = ref.flags_under(cols, vc, pb, t, par)
        cond = pd.Series(cols["volume_ratio"][:t + 1]) >= vc
        base = (cond.rolling(8, min_periods=1).sum() >= 2) & cond
        want = base & (~(base.shift(1) == True)) if mode == "first" else base   # noqa: E712
        assert (f["volume_cluster_flag"] == want.to_numpy()).all()
        seen += int(want.sum())
    assert seen >= 3
