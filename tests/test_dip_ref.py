"""CPU: the numpy / pandas restatement (tests/dip_ref.py) equals what the real
BuyTheDip.signal(), _allows_buy_the_dip_autotrade and _resolve_autotrade_route
did (tests/golden/dip_gates.npz, recorded by tests/golden/make_golden_dip.py).
Codes exact; values bit for bit with the recorded ema20 as input, ema20 at
1e-9 relative with the restatement's own ewm."""

import numpy as np

from tests import dip_cases as dc
from tests.dip_cases import pg, ref


def test_fixture_is_what_it_is_for():
    fx, p = dc.fixture(), dc.panel()
    status = fx["status"]
    assert status.shape == (pg.S, pg.T) == p["close"].shape
    counts = np.bincount(status.ravel(), minlength=8)
    assert len(counts) == 8 and (counts >= 20).all(), counts
    assert (p["first_t"] > 0).sum() >= 3
    assert list(fx["default_names"]) == list(ref.DEFAULTS)
    assert fx["defaults"].tolist() == [float(v) for v in ref.DEFAULTS.values()]
    assert dict(zip(fx["class_names"].tolist(), fx["class_constants"].tolist())) == {
        k: ref.DEFAULTS[k] for k in ("lookback_candles", "lookback_ms", "start_time_ms")}
    assert tuple(fx["reasons"]) == ref.ROUTE_REASONS
    assert "market_regime_none" in ref.ROUTE_REASONS
    # the close_time grid straddles START_TIME
    assert (p["close_time"] < ref.DEFAULTS["start_time_ms"]).any() and (
        p["close_time"] >= ref.DEFAULTS["start_time_ms"]).any()
    # what the search is for: references off t - 24, across one and two step edges
    idx = dc.ref_replay(p, **dc.fixture_kwargs(True))["reference_index"]
    t = np.arange(pg.T)[None, :]
    found = idx >= 0
    assert (found & (idx != t - 24)).any(axis=1).sum() >= 3
    assert (found & (idx // 64 < t // 64)).sum() >= 3 and (found & (idx // 64 <= t // 64 - 2)).sum() >= 1
    # the edge values: a NaN close mid-frame, infinite closes at both ends of an emitted message, alone, a zero
    close = p["close"]
    for s, u in pg.NAN_CLOSE:
        assert (status[s, u:p["lens"][s]] == ref.NOT_READY).all() and (status[s, :u] != ref.NOT_READY).any()
    s, u, m = pg.INF_BOTH
    assert status[s, m] == ref.EMIT and np.isinf(close[s, m]) and np.isinf(fx["reference_price"][s, m])
    assert np.isnan(fx["change_6h"][s, m])
    assert status[pg.INF_ALONE] == ref.OUT_OF_BAND and np.isinf(fx["change_6h"][pg.INF_ALONE])
    zs, zt = pg.ZERO_CLOSE
    hit = fx["reference_price"][zs] == 0.0
    assert hit.any() and (fx["change_6h"][zs][hit] == 0.0).all() and (status[zs][hit] == ref.OUT_OF_BAND).all()
    # both autotrade verdicts among the emitted messages
    emit = status == ref.EMIT
    assert fx["autotrade"][emit].sum() >= 3 and (~fx["autotrade"][emit]).sum() >= 3
    assert not fx["autotrade"][~emit].any()


def test_replay_with_recorded_ema_is_exact():
    got = dc.ref_replay(dc.panel(), **dc.fixture_kwargs(with_ema=True))
    want = dc.recorded()
    dc.assert_codes_equal(got, want, "restatement")
    dc.assert_values_bits(got, want, "restatement")


def test_replay_with_own_ewm():
    got = dc.ref_replay(dc.panel(), **dc.fixture_kwargs(with_ema=False))
    want = dc.recorded()
    dc.assert_codes_equal(got, want, "restatement, own ewm")
    dc.assert_values_bits(got, want, "restatement, own ewm", names=dc.POINTWISE)
    dc.assert_ema_close(got, want, "restatement, own ewm")


def test_reverse_scan_is_the_largest_index():
    """find_reference on ascending times = the last index at or before the target."""
    rng = np.random.default_rng(4)
    ct = np.cumsum(rng.integers(1, 50, 300)).tolist()
    for first, t, target in ((0, 299, ct[150]), (10, 200, ct[10]), (10, 200, ct[10] - 1), (5, 5, ct[5]),
                             (0, 100, ct[100] + 7), (20, 250, ct[77] + 0)):
        want = max((u for u in range(first, t + 1) if ct[u] <= target), default=-1)
        assert ref.find_reference(ct, first, t, target) == want


def test_split_frames_equal_the_whole():
    """The method keeps no state: a replay split through lens / from_t equals the whole."""
    p = dc.panel()
    kw = dc.fixture_kwargs(with_ema=False)
    whole = dc.ref_replay(p, **kw)
    for k in (63, 64, 65):
        a = dc.ref_replay(p, **{**kw, "lens": np.minimum(p["lens"], k)})
        b = dc.ref_replay(p, **kw, from_t=np.full(pg.S, k))
        joined = np.concatenate([a["status"][:, :k], b["status"][:, k:]], axis=1)
        assert (joined == whole["status"]).all(), k


def test_routing_table_is_exact():
    fx, cs = dc.fixture(), pg.routing_cases()
    auto, reason = ref.routing(cs["context_ok"], cs["transitioning"], cs["stress"], cs["market_regime"],
                               cs["features_ok"], cs["micro_regime"])
    assert reason.tolist() == fx["routing_reason"].tolist()
    assert auto.tolist() == fx["routing_autotrade"].tolist()
    # the two methods disagree on purpose
    R = ref.ROUTE_REASONS.index("symbol_regime_unavailable")
    un = fx["routing_reason"] == R
    assert fx["routing_autotrade"][un & ~cs["features_ok"]].all()
    assert (un & cs["features_ok"]).any() and not fx["routing_autotrade"][un & cs["features_ok"]].any()


def test_emitted_routes_equal_the_routing_restatement():
    """The route and flag of every emitted message of the panel."""
    fx, p = dc.fixture(), dc.panel()
    kind = p["market_kind"]
    ctx_ok = (kind != pg.MARKET_KINDS.index("none"))[None, :]
    feats_ok = np.array(pg.IN_SNAPSHOT)[:, None] & ctx_ok
    auto, reason = ref.routing(ctx_ok, p["transitioning"][None, :], p["stress"][None, :], p["market_regime"][None, :],
                               feats_ok, p["micro_regime"])
    emit = fx["status"] == ref.EMIT
    assert (reason[emit] == fx["route"][emit]).all() and (auto[emit] == fx["autotrade"][emit]).all()
