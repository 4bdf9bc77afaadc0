"""CPU: the numpy restatement (tests/bbextreme_ref.py) equals what the real
BBExtremeReversion.signal(), supports_autotrade and
_resolve_directional_autotrade did (tests/golden/bbextreme_gates.npz, recorded
by tests/golden/make_golden_bbextreme.py). Codes exact, values bit for bit:
the restatement performs the method's IEEE operations in its order, pandas'
roll_mean included. The direct-sum shortcut does not equal the recording."""

import numpy as np
import pytest

from tests import bbextreme_cases as bc
from tests.bbextreme_cases import pg, ref


def test_fixture_is_what_it_is_for():
    fx, p = bc.fixture(), bc.panel()
    assert fx["windows"].tolist() == list(bc.WINDOWS)
    assert list(fx["default_names"]) == list(ref.DEFAULTS)
    assert fx["defaults"].tolist() == [float(v) for v in ref.DEFAULTS.values()]
    assert tuple(fx["reasons"]) == ref.ROUTE_REASONS
    assert (p["first_t"] > 0).sum() >= 3 and (p["lens"] < pg.T).sum() >= 3
    for window in bc.WINDOWS:
        rec = bc.recorded(window)
        status = rec["status"]
        assert status.shape == (pg.S, pg.T) == p["close"].shape
        counts = np.bincount(status.ravel(), minlength=7)
        assert len(counts) == 7 and (counts >= 20).all(), counts
        emit = status == ref.EMIT
        assert (rec["direction"][emit] == ref.BUY).sum() >= 3 and (rec["direction"][emit] == ref.SELL).sum() >= 3
        assert np.isnan(rec["direction"][~emit]).all() and not rec["autotrade"][~emit].any()
        # NO_RSI carries evaluate's 50.0; a NaN span falls through to NO_EXTREME at band_position 0.5
        assert (rec["rsi_value"][status == ref.NO_RSI] == 50.0).all()
        span = p["bb_upper"] - p["bb_lower"]
        fell = np.isnan(span) & (status == ref.NO_EXTREME)
        assert fell.sum() >= 3 and (rec["band_position"][fell] == 0.5).all()
        assert (rec["band_position"][status == ref.INVALID_BAND] == 0.5).all()
        reached = emit | (status >= ref.NO_RSI)
        dead_mid = reached & ~(p["bb_mid"] > 0)
        assert dead_mid.sum() >= 3 and (rec["bb_width"][dead_mid] == 0.0).all()
        assert (rec["distance_from_mid_pct"][dead_mid] == 0.0).all()
        # an infinite close is a value to the null gate
        assert (np.isinf(p["close"]) & (status == ref.NO_RSI)).any()
        assert (np.isnan(p["close"]) & (status == ref.NULLS)).any()


@pytest.mark.parametrize("window", bc.WINDOWS)
def test_replay_is_bit_exact(window):
    got, want = bc.fixture_replay(window), bc.recorded(window)
    bc.assert_codes_equal(got, want, f"restatement, rsi_window {window}")
    bc.assert_values_bits(got, want, f"restatement, rsi_window {window}")


def test_direct_sums_are_not_the_method():
    """The RSI formed from the last window's own sums differs from the
    recording at 20 cells or more, at frames across a 64-candle edge too, and
    changes the decision at one or more."""
    want, direct = bc.recorded(2), bc.fixture_replay(2, direct=True)
    reached = (want["status"] == ref.EMIT) | (want["status"] >= ref.NO_RSI)
    differs = reached & ~bc.same_bits(want["rsi_value"], direct["rsi_value"])
    t = np.arange(pg.T)[None, :]
    assert differs.sum() >= 20 and (differs & (t // 64 != (t - 29) // 64)).sum() >= 3
    assert (direct["status"] != want["status"]).sum() >= 1
    with pytest.raises(AssertionError):
        bc.assert_values_bits(direct, want, names=("rsi_value",))


def test_roll_mean_rules_hit_on_the_fixture():
    """The consecutive-same-value rule, the no-negative sign rule and the
    missing-observation rule form means of the panel. The all-negative sign
    rule cannot: a window of the method's holds the sign bit only on losses of
    -0.0, which are all equal, and the same-value rule answers first."""
    rule = bc.fixture_replay(2)["mean_rule"]
    seen = np.bincount(rule[rule >= 0].ravel(), minlength=5)
    assert seen[ref.SAME_VALUE] >= 20 and seen[ref.NO_NEGATIVE] >= 3 and seen[ref.TOO_FEW] >= 3, seen
    assert seen[ref.ALL_NEGATIVE] == 0
    # the rule itself, on values the method cannot produce
    assert ref.roll_mean_last([-157245200.0, -1.5416160486402442e+17, -1.3163965927504378e+16, -1947.0,
                               -16364673393523.0, -3.0, -1.0], 2) == (0.0, ref.ALL_NEGATIVE)


def test_roll_mean_by_hand():
    """calc_mean's branches on small inputs (pandas 2.3.3's results)."""
    nan = float("nan")
    assert ref.roll_mean_last([0.0, 0.0, 0.0], 2) == (0.0, ref.SAME_VALUE)
    m, r = ref.roll_mean_last([-0.0, -0.0, -0.0], 2)
    assert r == ref.SAME_VALUE and np.signbit(m)
    assert ref.roll_mean_last([0.0, 1.0, 3.0], 2) == (2.0, ref.PLAIN)
    m, r = ref.roll_mean_last([0.0, float("inf"), 3.0], 2)
    assert m != m and r == ref.TOO_FEW
    assert ref.roll_mean_last([0.0, float("inf"), 3.0, 5.0], 2) == (4.0, ref.PLAIN)   # the chain skips the missing row
    assert ref.roll_mean_last([0.1, 0.1, 0.1], 3) == (0.1, ref.SAME_VALUE)            # not 0.10000000000000002
    assert ref.frame_rsi([1.0, 2.0], 2) is None and ref.frame_rsi([1.0, 2.0, 3.0], 2) == 100.0
    assert ref.frame_rsi([3.0, 2.0, 1.0], 2) == 0.0 and ref.frame_rsi([1.0, 1.0, 1.0], 2) is None
    assert ref.frame_rsi([1.0, 2.0, float("inf")], 2) is None and ref.frame_rsi([nan, 2.0, 1.0, 3.0], 2) is not None


def test_split_frames_equal_the_whole():
    """The method keeps no state: a replay split through lens / from_t equals the whole."""
    p = bc.panel()
    whole = bc.fixture_replay(2)
    rows = slice(0, 12)
    q = {k: p[k][rows] for k in ("close",) + bc.BANDS}
    for k in (63, 64, 65):
        a = bc.ref_replay(q, first_t=p["first_t"][rows], lens=np.minimum(p["lens"][rows], k))
        b = bc.ref_replay(q, first_t=p["first_t"][rows], lens=p["lens"][rows], from_t=np.full(12, k))
        joined = np.concatenate([a["status"][:, :k], b["status"][:, k:]], axis=1)
        assert (joined == whole["status"][rows]).all(), k


def test_routing_table_is_exact():
    fx, cs = bc.fixture(), pg.routing_cases()
    auto, route = ref.routing(cs["context_ok"], cs["transitioning"], cs["timestamp"], cs["stable_since"], cs["stress"],
                              cs["market_regime"], cs["features_ok"], cs["micro_regime"], cs["micro_transition"],
                              cs["strength"], cs["direction"])
    assert route.tolist() == fx["routing_reason"].tolist()
    assert auto.tolist() == fx["routing_autotrade"].tolist()
    R = ref.ROUTE_REASONS.index
    # the methods' quirks: a NaN strength passes; a None micro regime is not shortable, and fine for a buy
    passed = fx["routing_autotrade"]
    assert (passed & np.isnan(cs["strength"])).any()
    none_micro = cs["features_ok"] & (cs["micro_regime"] < 0) & cs["context_ok"]
    assert (fx["routing_reason"][none_micro & (cs["direction"] == ref.SELL)] != R("market_range_stable")).all()
    assert (passed & none_micro & (cs["direction"] == ref.BUY)).any()
    assert not (passed & none_micro & (cs["direction"] == ref.SELL)).any()
    assert set(fx["routing_reason"][passed].tolist()) == {R("market_range_unstable_allowed"), R("market_range_stable")}


@pytest.mark.parametrize("window", bc.WINDOWS)
def test_emitted_routes_equal_the_routing_restatement(window):
    """The route and flag of every emitted message of the panel."""
    p, rec = bc.panel(), bc.recorded(window)
    ctx_ok = (p["market_kind"] != pg.MARKET_KINDS.index("none"))[None, :]
    feats_ok = np.array(pg.IN_SNAPSHOT)[:, None] & ctx_ok
    auto, route = ref.routing(ctx_ok, p["transitioning"][None, :], p["timestamp"][None, :], p["stable_since"][None, :],
                              p["stress"][None, :], p["market_regime"][None, :], feats_ok, p["micro_regime"],
                              p["micro_transition"], p["strength"], rec["direction"])
    emit = rec["status"] == ref.EMIT
    assert (route[emit] == rec["route"][emit]).all() and (auto[emit] == rec["autotrade"][emit]).all()
