"""CPU: the numpy restatement of LiquidationSweepPump's gate, rank, routing and
the selector's pick (tests/sweep_ref.py) equals the fixture recorded from the
real signal() (tests/golden/sweep_gates.npz, make_golden_sweep.py) exactly, in
every section."""

import numpy as np

from tests import sweep_cases as sc
from tests.sweep_cases import pg, ref


def _select(route=True, rank="names"):
    fx, p = sc.fixture(), sc.panel()
    cols, cross = sc.fixture_columns()
    return ref.select(cols, cross, route_ok=p["route_ok"] if route else None, first_t=p["first_t"], lens=p["lens"],
                      symbol_rank=ref.symbol_ranks(fx["names"]) if rank == "names" else None)


def test_fixture_is_what_the_restatement_states():
    fx = sc.fixture()
    assert tuple(fx["columns"]) == ref.COLUMNS and tuple(fx["reasons"]) == ref.REASONS
    assert tuple(fx["route_reasons"]) == ref.ROUTE_REASONS and tuple(fx["names"]) == pg.NAMES
    assert dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist())) == {k: float(v) for k, v in
                                                                                 ref.DEFAULTS.items()}
    ranks = ref.symbol_ranks(pg.NAMES)
    assert sorted(pg.NAMES) == [pg.NAMES[i] for i in np.argsort(ranks)]
    assert (ranks != np.arange(pg.S)).any()   # the str order is not the row order


def test_candidates_and_rank_scores_equal_signal():
    fx = sc.fixture()
    got = _select()
    assert got["candidate"].tolist() == fx["submitted"].tolist()
    assert sc.same_bits(got["rank_score"], fx["rank_score"]).all()
    assert fx["submitted"].sum() >= 40


def test_status_agrees_with_the_stage_signal_stopped_at():
    """is_candidate / route_reason record how far signal() went at each cell."""
    fx, p = sc.fixture(), sc.panel()
    st = _select()["status"]
    u = np.arange(pg.T)[None, :]
    message = (u + 1 < p["lens"][:, None]) & (u >= p["first_t"][:, None])
    assert ((st == ref.NO_FRAME) == ~message).all()
    assert ((st == ref.SHORT_FRAME) == (message & (u + 2 - p["first_t"][:, None] < ref.DEFAULTS["min_frame"]))).all()
    reached = message & (st != ref.SHORT_FRAME)
    assert ((fx["is_candidate"] >= 0) == reached).all()   # _is_candidate ran exactly past the frame gate
    gate_fail = (st >= ref.NOT_FINITE) & (st <= ref.BTC_TREND)
    assert (gate_fail == (fx["is_candidate"] == 0)).all()
    assert ((st == ref.THRESHOLD_NONPOSITIVE) == ((fx["is_candidate"] == 1) & (fx["route_reason"] == 255))).all()
    assert ((st == ref.ROUTE_REFUSED) == ((fx["route_reason"] != 255) & (fx["route_reason"] != ref.ROUTE_OK))).all()
    counts = np.bincount(st.ravel(), minlength=256)
    assert (counts[:15] >= 5).all() and counts[ref.NO_FRAME] >= 5, counts[:15]


def test_winners_equal_the_selector_dispatch():
    fx = sc.fixture()
    got = _select()
    assert got["winner"].tolist() == fx["dispatched"].tolist()
    assert sc.same_bits(got["winner_score"], fx["dispatched_score"]).all()
    per_col = fx["submitted"].sum(axis=0)
    assert (per_col >= 2).sum() >= 8
    # the symbol tie-break: by row index the tie cohorts pick another row, with the same score
    by_row = _select(rank=None)
    differ = np.flatnonzero(by_row["winner"] != got["winner"])
    assert len(differ) >= 1 and sc.same_bits(by_row["winner_score"], got["winner_score"]).all()
    top = np.where(fx["submitted"], fx["rank_score"], -np.inf)
    tied = [t for t in range(pg.T) if per_col[t] >= 2 and (top[:, t] == top[:, t].max()).sum() >= 2]
    assert len(tied) >= 2 and set(differ) <= set(tied)


def test_without_routing_the_refused_cells_are_candidates():
    st, plain = _select()["status"], _select(route=False)["status"]
    refused = st == ref.ROUTE_REFUSED
    assert refused.sum() >= 5 and (plain[refused] == 0).all() and (plain[~refused] == st[~refused]).all()


def test_no_gate_decision_on_a_near_tie():
    p = sc.panel()
    cols, cross = sc.fixture_columns()
    assert sc.near_ties(cols, cross, first_t=p["first_t"], lens=p["lens"]) == 0


def test_routing_grid():
    fx = sc.fixture()
    cases = pg.routing_cases()
    latest, recovery = np.array([pg.breadth_inputs(c) for c in cases]).T
    got = ref.routing([c["stress"] for c in cases], latest, recovery, [c["context_ok"] for c in cases],
                      [c["btc_momentum"] for c in cases], [c["trend"] for c in cases],
                      [c["features_ok"] for c in cases])
    assert got.tolist() == fx["routing_reason"].tolist()
    assert (np.bincount(got, minlength=len(ref.ROUTE_REASONS)) >= 4).all()
    assert any(len(c["breadth"]) == 2 for c in cases) and any(not c["context_ok"] for c in cases)
    # the panel's stand-in refusals are refusals, its benign case is not
    for kind in range(len(pg.REFUSALS)):
        c = pg.route_case_at(False, kind)
        b, r = pg.breadth_inputs(c)
        assert ref.routing(c["stress"], b, r, c["context_ok"], 0.001, c["trend"], c["features_ok"]) != ref.ROUTE_OK
    b, r = pg.breadth_inputs(pg.BENIGN)
    assert ref.routing(pg.BENIGN["stress"], b, r, True, 0.001, pg.BENIGN["trend"], True) == ref.ROUTE_OK


def test_reference_test_frames():
    fx = sc.fixture()
    assert fx["frame_names"].tolist() == ["emits_long", "symbol_trend_not_up", "btc_not_increasing"]
    cols = {k: fx["frame_values"][:, i:i + 1] for i, k in enumerate(ref.COLUMNS)}
    n = len(fx["frame_names"])
    # one column per frame: the trigger candle df.iloc[-2] of a frame of frame_len candles
    status = np.array([ref.gate({k: v[i:i + 1] for k, v in cols.items()}, fx["frame_cross"][i:i + 1, None],
                                first_t=[-(int(fx["frame_len"][i]) - 2)], lens=[2])[0][0, 0] for i in range(n)])
    stress, breadth, recovery, btc, trend = fx["frame_route_in"].T
    reason = ref.routing(stress, breadth, recovery, np.ones(n, bool), btc, trend, np.ones(n, bool))
    assert reason.tolist() == fx["frame_reason"].tolist()
    emitted = (status == 0) & (reason == ref.ROUTE_OK)
    assert emitted.tolist() == fx["frame_emitted"].tolist() == [True, False, False]
    # the third frame's btc_momentum_3 of 0 already fails _is_candidate (:298)
    assert status.tolist() == [0, 0, ref.BTC_MOMENTUM]
