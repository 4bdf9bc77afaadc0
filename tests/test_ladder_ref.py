"""CPU: the numpy restatement (tests/ladder_ref.py) reproduces what the real
LadderDeployer.signal() did
(tests/golden/ladder_gates.npz, recorded by tests/golden/make_golden_ladder.py):
every status code and every value bit, at every cell, for the bands passed
unrounded and for the bands rounded to 6 places by the caller."""

import numpy as np
import pytest

from tests import ladder_cases as lc
from tests.ladder_cases import pg, ref


@pytest.mark.parametrize("recording", lc.RECORDINGS)
def test_restatement_reproduces_the_real_method(recording):
    want, got = lc.recorded(recording), lc.fixture_replay(recording)
    assert want["status"].shape == (pg.S, pg.T)
    lc.assert_codes_equal(got, want, recording)
    lc.assert_values_equal(got, want, recording)


def test_fixture_holds_what_it_is_for():
    """The generator's check_coverage, in short: every code, both clamps, the exact widths."""
    fx, p = lc.fixture(), lc.panel()
    assert tuple(fx["reasons"]) == ref.REASONS and tuple(fx["policy_reasons"]) == ref.POLICY_REASONS
    assert dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist())) == ref.DEFAULTS
    for recording in lc.RECORDINGS:
        rec = lc.recorded(recording)
        counts = np.bincount(rec["status"].ravel(), minlength=len(ref.REASONS))
        assert len(counts) == len(ref.REASONS) and (counts >= 20).all(), counts
        emit = rec["status"] == ref.EMIT
        for k in ref.VALUES[2:]:
            assert not np.isnan(rec[k][emit]).any() and np.isnan(rec[k][~emit]).all()
        sized = emit | (rec["status"] == ref.RANGE_WIDTH)
        assert not np.isnan(rec["range_width_pct"][sized]).any() and np.isnan(rec["range_width_pct"][~sized]).all()
    rec = lc.recorded("plain")
    emit = rec["status"] == ref.EMIT
    buf = rec["breakout_buffer_pct"]
    assert (emit & np.isnan(p["atr_pct"]) & (buf == 4.0)).any() and (emit & (buf == 0.5)).any()
    assert (emit & (rec["range_width_pct"] == 1.5)).any() and (emit & (rec["range_width_pct"] == 8.0)).any()
    r6 = lc.recorded("r6")
    assert ((r6["status"] == ref.RANGE_WIDTH) & (lc.rounded()["bb_mid_arg"] <= 0)).any()
    assert (rec["status"] != r6["status"]).any()
    assert (p["first_t"] > 0).any() and (p["lens"] < pg.T).any() and pg.T > ref.TILE + ref.DEFAULTS["n"]


def test_from_t_and_short_windows():
    """from_t only masks: the replayed candles keep their values; n = 1 never expands."""
    p = lc.panel()
    full = lc.fixture_replay("plain")
    frm = np.full(pg.S, pg.T - 1)
    last = lc.ref_replay(p, first_t=p["first_t"], lens=p["lens"], from_t=frm)
    assert (last["status"][:, :-1] == ref.NO_FRAME).all()
    for k in ("status",) + ref.VALUES:
        assert lc.same_bits(last[k][:, -1], full[k][:, -1]).all()
    one = lc.ref_replay(p, first_t=p["first_t"], lens=p["lens"], n=1)
    walked = (one["status"] == ref.EMIT) | (one["status"] >= ref.BB_EXPANDING)
    clean = walked & ~np.isnan(one["bb_change_pct"])
    assert (one["bb_change_pct"][clean] == 0.0).all() and (one["status"][clean] != ref.BB_EXPANDING).all()
