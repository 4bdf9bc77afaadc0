"""CPU: the numpy / pandas restatement (tests/pricetracker_ref.py) equals what
the real PriceTracker.signal(), regime_routing, allows_long_autotrade and
ActivityBurstPump.signal() did (tests/golden/pricetracker_gates.npz, recorded
by tests/golden/make_golden_pricetracker.py). Codes, detail bits and the
cooldown entries exact; values bit for bit with the recorded trend_score as
input, at 1e-9 with the restatement's own ewm."""

import numpy as np

from tests import pricetracker_cases as pc
from tests.pricetracker_cases import pg, ref


def test_fixture_is_what_it_is_for():
    fx, p = pc.fixture(), pc.panel()
    counts = np.bincount(fx["status"].ravel(), minlength=7)
    assert (counts >= 20).all(), counts
    assert all(((fx["detail"] & b) != 0).sum() >= 10 for b in (1, 2, 4))
    assert (fx["repeat_status"] == ref.COOLDOWN).sum() >= 3
    assert list(fx["default_names"]) == list(ref.DEFAULTS)
    assert fx["defaults"].tolist() == [float(v) for v in ref.DEFAULTS.values()]
    assert tuple(fx["reasons"]) == ref.ROUTE_REASONS
    assert fx["status"].shape == (pg.S, pg.T) == p["close"].shape


def test_replay_with_recorded_trend_is_exact():
    fx, p = pc.fixture(), pc.panel()
    got = pc.ref_replay(p, **pc.fixture_kwargs(with_trend=True))
    want = pc.recorded()
    pc.assert_codes_equal(got, want, "restatement")
    pc.assert_values_bits(got, want, "restatement")
    pc.assert_state_equal(got["state"], (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")


def test_replay_with_own_ewm():
    p = pc.panel()
    got = pc.ref_replay(p, **pc.fixture_kwargs(with_trend=False))
    want = pc.recorded()
    pc.assert_codes_equal(got, want, "restatement, own ewm")
    pc.assert_values_close(got, want, "restatement, own ewm")


def test_state_after_every_candle():
    """The cooldown entry after the message of candle k, for a few k: a replay
    of candles .. k from nothing, and one resumed from the recording at k - 1."""
    fx, p = pc.fixture(), pc.panel()
    for k in (57, 63, 64, 65, 130, 199):
        lens = np.minimum(p["lens"], k + 1)
        kw = {**pc.fixture_kwargs(with_trend=True), "lens": lens}
        got = pc.ref_replay(p, **kw)
        pc.assert_state_equal(got["state"], (fx["state_has"][:, k], fx["state_last"][:, k]), f"after candle {k}")
        resumed = pc.ref_replay(p, **kw, state=(fx["state_has"][:, k - 1], fx["state_last"][:, k - 1]),
                                from_t=np.full(pg.S, k))
        assert (resumed["status"][:, k] == fx["status"][:, k]).all()
        pc.assert_state_equal(resumed["state"], (fx["state_has"][:, k], fx["state_last"][:, k]), f"resumed at {k}")


def test_repeated_messages():
    fx, p = pc.fixture(), pc.panel()
    for i, (s, t) in enumerate(p["repeats"]):
        rows = slice(s, s + 1)
        kw = {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (pg.S,) else v)
              for k, v in pc.fixture_kwargs(with_trend=True).items()}
        kw["lens"] = np.array([t + 1])
        got = ref.replay(*(p[k][rows] for k in pc.PANELS), p["close_time"][rows], **kw, from_t=np.array([t]),
                         state=(fx["state_has"][rows, t], fx["state_last"][rows, t]))
        assert got["status"][0, t] == fx["repeat_status"][i], (s, t)
        assert got["state"][1][0] == fx["repeat_last"][i]


def test_routing_grid_is_exact():
    fx, cs = pc.fixture(), pg.routing_cases()
    got = ref.routing(cs["context_ok"], cs["transitioning"], cs["stress"], cs["advancers_ratio"], cs["long_tailwind"],
                      cs["short_tailwind"], cs["market_regime"], cs["features_ok"], cs["micro_regime"],
                      cs["micro_transition"], cs["rs"], cs["trend"])
    assert got.tolist() == fx["routing_reason"].tolist()


def test_autotrade_grid_is_exact():
    fx, cs = pc.fixture(), pg.autotrade_cases()
    got = ref.long_autotrade(cs["context_ok"], cs["transitioning"], cs["timestamp"], cs["stable_since"],
                             cs["market_regime"], cs["stress"], cs["features_ok"], cs["micro_regime"],
                             cs["micro_transition"])
    assert got.tolist() == fx["autotrade_allowed"].tolist()


def burst_inputs():
    """(qualified, route_ok [1, T], ctx_ok [T], first_t) of the recorded burst panel."""
    bp, cs = pg.burst_panel(), pg.autotrade_cases()
    idx = np.maximum(bp["case"], 0)
    allowed = ref.long_autotrade(*(cs[k][idx] for k in ("context_ok", "transitioning", "timestamp", "stable_since",
                                                         "market_regime", "stress", "features_ok", "micro_regime",
                                                         "micro_transition")))
    ctx_ok = (bp["case"] >= 0) & cs["context_ok"][idx]
    return bp["qualified"], allowed[None, :], ctx_ok, bp["first_t"]


def test_burst_entry_is_exact():
    fx = pc.fixture()
    q, route, ctx_ok, first = burst_inputs()
    status, autotrade = ref.burst_entry(q, route, ctx_ok, first_t=first)
    assert ((status == ref.AB_EMIT) == fx["burst_emitted"]).all()
    assert (autotrade == fx["burst_autotrade"]).all()
    assert all((status == c).any() for c in range(5))
