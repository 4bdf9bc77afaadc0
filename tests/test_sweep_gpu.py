"""LiquidationSweepPump's candidate gate and the cohort winner on the device
(signals.liquidation_sweep_select, bq_sweep.hip): against the REAL signal()'s
outcomes (tests/golden/sweep_gates.npz) and, at the edges of the kernel's two
mappings, against the restatement that fixture pins (tests/sweep_ref.py).
Status exact, rank_score bit for bit, winner and winner_score exact."""

import numpy as np
import pytest
import torch

from tests import sweep_cases as sc
from tests.sweep_cases import pg, ref

pytestmark = pytest.mark.gpu

TILE, CHUNK, SWITCH = sc.TILE, sc.ROW_CHUNK, sc.SWITCH


def dv(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def dcols(cols, pad=0):
    """The columns on the device; pad > 0: [S, T] views of [S, T + pad] buffers."""
    out = {}
    for k in ref.COLUMNS:
        a = np.asarray(cols[k], np.float64)
        if pad:
            buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float64, device="cuda")
            buf[:, :a.shape[1]] = dv(a)
            out[k] = buf[:, :a.shape[1]]
        else:
            out[k] = dv(a)
    return out


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def device_select(cols, cross, route=None, first_t=None, lens=None, rank=None, t_range=None, pad=0):
    from binquant_amd import signals

    d = dcols(cols, pad)
    d["score_cross"] = dv(cross, bool)
    return host(signals.liquidation_sweep_select(
        d, route_ok=dv(route, bool), first_t=dv(first_t, np.int64), lens=dv(lens, np.int64),
        symbol_rank=dv(rank, np.int32), t_range=t_range))


def assert_select_equal(got, want, what="", t_range=None):
    lo, hi = t_range or (0, want["status"].shape[1])
    g, w = got["status"][:, lo:hi], want["status"][:, lo:hi]
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: status differs at {bad[:5].tolist()}: " \
                          f"{[(int(g[tuple(i)]), int(w[tuple(i)])) for i in bad[:5]]}"
    assert (got["candidate"][:, lo:hi] == (w == 0)).all(), what
    eq = sc.same_bits(got["rank_score"][:, lo:hi], want["rank_score"][:, lo:hi])
    assert eq.all(), f"{what}: rank_score differs at {np.argwhere(~eq)[:5].tolist()}"
    bad = np.flatnonzero(got["winner"][lo:hi] != want["winner"][lo:hi])
    assert len(bad) == 0, f"{what}: winner differs at columns {(bad[:5] + lo).tolist()}: " \
                          f"{got['winner'][lo:hi][bad[:5]].tolist()} != {want['winner'][lo:hi][bad[:5]].tolist()}"
    assert sc.same_bits(got["winner_score"][lo:hi], want["winner_score"][lo:hi]).all(), f"{what}: winner_score"


# ---- the fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [True, False], ids=["route", "no_route"])
@pytest.mark.parametrize("rank", ["names", None], ids=["by_name", "by_row"])
def test_fixture_panel(cuda, route, rank):
    fx, p = sc.fixture(), sc.panel()
    cols, cross = sc.fixture_columns()
    kw = dict(route=p["route_ok"] if route else None, first_t=p["first_t"], lens=p["lens"],
              rank=ref.symbol_ranks(fx["names"]) if rank else None)
    got = device_select(cols, cross, **kw)
    want = ref.select(cols, cross, route_ok=kw["route"], first_t=kw["first_t"], lens=kw["lens"],
                      symbol_rank=kw["rank"])
    assert_select_equal(got, want, "fixture")
    if route:   # the recorded outcomes of the real signal() and selector
        assert (got["candidate"] == fx["submitted"]).all()
        assert sc.same_bits(got["rank_score"], fx["rank_score"]).all()
        tied = np.flatnonzero(ref.winners(want["status"], want["rank_score"], None)[0]
                              != ref.winners(want["status"], want["rank_score"], ref.symbol_ranks(fx["names"]))[0])
        assert len(tied) >= 1
        if rank:
            assert (got["winner"] == fx["dispatched"]).all()
            assert sc.same_bits(got["winner_score"], fx["dispatched_score"]).all()
        else:   # NULL symbol_rank: the tie cohorts go to the larger row, the same score
            assert (got["winner"][tied] != fx["dispatched"][tied]).all()
            others = np.setdiff1d(np.arange(pg.T), tied)
            assert (got["winner"][others] == fx["dispatched"][others]).all()
            assert sc.same_bits(got["winner_score"], fx["dispatched_score"]).all()


# ---- the wide mapping (lane = candle) ----------------------------------------------------------------------------
def _ragged(S, T, g):
    first = np.where(g.random(S) < 0.3, g.integers(0, max(T // 2, 1), S), 0)
    lens = np.where(g.random(S) < 0.3, g.integers(max(T // 2, 1), T + 1, S), T)
    return first.astype(np.int64), lens.astype(np.int64)


@pytest.mark.parametrize("S,T,pad", [(70, TILE - 1, 0), (70, TILE, 0), (70, TILE + 1, 0), (CHUNK - 1, 300, 0),
                                     (CHUNK, 300, 0), (CHUNK + 1, 300, 0), (1, 300, 0), (3 * CHUNK + 5, 2 * TILE + 9, 24),
                                     (5, SWITCH, 0)])
def test_wide_shapes(cuda, S, T, pad):
    g = np.random.default_rng(1000 * S + T)
    cols, cross, route = sc.planted_columns(S, T, seed=S * 7919 + T)
    first, lens = _ragged(S, T, g)
    rank = g.permutation(S).astype(np.int32)
    got = device_select(cols, cross, route, first, lens, rank, pad=pad)
    want = ref.select(cols, cross, route_ok=route, first_t=first, lens=lens, symbol_rank=rank)
    assert_select_equal(got, want, f"S={S} T={T}")
    if S > 1 and T > 200:
        assert (want["winner"] >= 0).sum() > 10 and (want["status"] == 0).sum() > 10


def test_wide_planted_edges(cuda):
    """The only candidate of a column in the first / last row of a chunk, a
    column with none, +inf beating a finite score, one score in two chunks
    resolved by the rank, equal ranks resolved by the row."""
    S, T = 2 * CHUNK + 2, TILE + 40
    cols, cross, _ = sc.planted_columns(S, T, seed=5)
    rank = np.arange(S, dtype=np.int32)[::-1].copy()   # the str order reversed: the smaller row wins a tie
    for t in range(60, 72):
        sc.clear_column(cols, cross, t)
    sc.plant(cols, cross, None, CHUNK, 60)            # first row of the second chunk
    sc.plant(cols, cross, None, 2 * CHUNK - 1, 61)    # last row of the second chunk
    sc.plant(cols, cross, None, 0, 62)
    sc.plant(cols, cross, None, S - 1, 63)            # the last row, in the ragged third chunk
    sc.plant(cols, cross, None, 3, 65, np.inf)
    sc.plant(cols, cross, None, 100, 65, 1e6)
    sc.plant(cols, cross, None, 10, 66, 7.0)
    sc.plant(cols, cross, None, 70, 66, 7.0)
    sc.plant(cols, cross, None, 11, 67, 9.0)
    sc.plant(cols, cross, None, 12, 67, 9.0)
    sc.plant(cols, cross, None, 90, 67, 9.0)
    dup = rank.copy()
    dup[[11, 12, 90]] = 5                             # duplicate ranks (a caller error): the larger row
    for r, name in ((rank, "reversed"), (dup, "duplicate"), (None, "row")):
        got = device_select(cols, cross, rank=r)
        want = ref.select(cols, cross, symbol_rank=r)
        assert_select_equal(got, want, name)
        w = got["winner"]
        assert w[60] == CHUNK and w[61] == 2 * CHUNK - 1 and w[62] == 0 and w[63] == S - 1
        assert w[64] == -1 and np.isnan(got["winner_score"][64])
        assert w[65] == 3 and np.isposinf(got["winner_score"][65])
        assert w[66] == (70 if r is None else 10)
        assert w[67] == (11 if name == "reversed" else 90)


# ---- the narrow mapping (lane = row) -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_narrow_shapes(cuda, S):
    """One column and a few: the winner in the last lane of the last partial
    wave, NO_FRAME rows around it; equal to that column of a full-range call."""
    T = 80
    g = np.random.default_rng(S)
    cols, cross, route = sc.planted_columns(S, T, seed=S + 31, density=0.3)
    first, lens = np.zeros(S, np.int64), np.full(S, T, np.int64)
    u = 70
    sc.plant(cols, cross, route, S - 1, u, 1e9)        # beats every planted score
    if S > 3:
        first[S - 2], lens[S - 3] = u + 1, u + 1       # no message around the winner
        first[0] = u + 5
    rank = g.permutation(S).astype(np.int32)
    want = ref.select(cols, cross, route_ok=route, first_t=first, lens=lens, symbol_rank=rank)
    assert want["winner"][u] == S - 1
    full = device_select(cols, cross, route, first, lens, rank)           # T >= SWITCH: the wide mapping
    assert_select_equal(full, want, f"S={S} full")
    for lo, hi in ((u, u + 1), (u - 3, u + 4), (T - SWITCH + 1, T)):
        got = device_select(cols, cross, route, first, lens, rank, t_range=(lo, hi))
        assert_select_equal(got, want, f"S={S} [{lo}, {hi})", (lo, hi))
        assert (got["status"][:, lo:hi] == full["status"][:, lo:hi]).all()
        assert sc.same_bits(got["rank_score"][:, lo:hi], full["rank_score"][:, lo:hi]).all()
        assert (got["winner"][lo:hi] == full["winner"][lo:hi]).all()
        assert sc.same_bits(got["winner_score"][lo:hi], full["winner_score"][lo:hi]).all()


def test_narrow_column_without_a_candidate(cuda):
    S, T = 130, 70
    cols, cross, _ = sc.planted_columns(S, T, seed=77)
    sc.clear_column(cols, cross, 65)
    got = device_select(cols, cross, t_range=(65, 66))
    assert got["winner"][65] == -1 and np.isnan(got["winner_score"][65])
    assert (got["status"][:, 65] != 0).all() and np.isnan(got["rank_score"][:, 65]).all()


# ---- the range ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(70, 71), (60, 90), (10, 10 + TILE + 3), (0, 0)])
def test_range_is_honoured(cuda, lo, hi):
    from binquant_amd import engine

    S, T = 70, 300
    cols, cross, route = sc.planted_columns(S, T, seed=9)
    d = dcols(cols)
    out = dict(status=torch.full((S, T), 0xEE, dtype=torch.uint8, device="cuda"),
               rank_score=torch.full((S, T), -123.0, dtype=torch.float64, device="cuda"),
               winner=torch.full((T,), -77, dtype=torch.int64, device="cuda"),
               winner_score=torch.full((T,), -5.0, dtype=torch.float64, device="cuda"))
    engine.sweep_select([d[k] for k in ref.COLUMNS], dv(cross, bool), route_ok=dv(route, bool), t_range=(lo, hi),
                        out=out)
    got = host(out)
    want = ref.select(cols, cross, route_ok=route)
    outside = np.ones(T, bool)
    outside[lo:hi] = False
    assert (got["status"][:, outside] == 0xEE).all() and (got["rank_score"][:, outside] == -123.0).all()
    assert (got["winner"][outside] == -77).all() and (got["winner_score"][outside] == -5.0).all()
    got["candidate"] = got["status"] == 0
    assert_select_equal(got, want, f"[{lo}, {hi})", (lo, hi))


# ---- routing --------------------------------------------------------------------------------------------------------
def test_routing_equals_the_fixture_grid(cuda):
    from binquant_amd import signals

    assert signals.SW_ROUTE_REASONS == ref.ROUTE_REASONS and tuple(signals.SW_REASONS.values()) == ref.REASONS
    fx = sc.fixture()
    cases = pg.routing_cases()
    latest, recovery = np.array([pg.breadth_inputs(c) for c in cases]).T
    row = lambda v, dt=np.float64: dv(np.asarray(v, dt).reshape(1, -1))   # noqa: E731
    ok, reason = signals.sweep_routing_allows(
        row([c["stress"] for c in cases]), row(latest), row(recovery), row([c["context_ok"] for c in cases], bool),
        row([c["btc_momentum"] for c in cases]), row([c["trend"] for c in cases]),
        row([c["features_ok"] for c in cases], bool))
    assert reason.cpu().numpy().ravel().tolist() == fx["routing_reason"].tolist()
    assert (ok.cpu().numpy().ravel() == (fx["routing_reason"] == ref.ROUTE_OK)).all()


# ---- graph capture ----------------------------------------------------------------------------------------------------
def test_select_graph_replays_on_changed_inputs(cuda):
    from binquant_amd import signals
    from binquant_amd.graphs import CapturedPipeline

    S, T = 200, 300
    rank = dv(np.random.default_rng(3).permutation(S), np.int32)

    def tensors(seed):
        cols, cross, route = sc.planted_columns(S, T, seed=seed)
        return [dv(cols[k]) for k in ref.COLUMNS] + [dv(cross, bool), dv(route, bool)]

    def fn(*a):
        d = dict(zip(ref.COLUMNS, a[:13]), score_cross=a[13])
        wide = signals.liquidation_sweep_select(d, route_ok=a[14], symbol_rank=rank)
        one = signals.liquidation_sweep_select(d, route_ok=a[14], symbol_rank=rank, t_range=(T - 2, T - 1))
        return {**{f"wide.{k}": v for k, v in wide.items()},
                **{f"one.{k}": v[..., T - 2:T - 1] for k, v in one.items()}}

    g = CapturedPipeline(fn, *tensors(1))
    b = tensors(2)
    got = {k: v.clone() for k, v in g(*b).items()}
    want = fn(*b)
    torch.cuda.synchronize()
    for k in want:
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=k)
    assert (want["wide.winner"] >= 0).sum() > 10


def _cohort_inputs(shift, T):
    p = sc.panel()
    roll = lambda a: np.roll(a, shift, axis=0)[:, :T]   # noqa: E731
    panel = [dv(roll(p[k])) for k in ("open", "high", "low", "close", "volume")]
    ts = p["open_time"][:T]
    return panel + panel + [dv(np.broadcast_to(ts, (pg.S, T))), dv(ts), dv(p["btc_close"][:T])]


def test_cohort_sweep_equals_the_select_and_leaves_the_default_alone(cuda):
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    fx, p = sc.fixture(), sc.panel()
    # the cohort whose trigger column T - 2 is the last one with a candidate among the rows that start at 0
    T = int(np.flatnonzero(fx["submitted"][p["first_t"] == 0].any(axis=0))[-1]) + 2
    ins, other = _cohort_inputs(0, T), _cohort_inputs(3, T)
    route = dv(p["route_ok"][:, T - 2], bool)
    rank = dv(ref.symbol_ranks(pg.NAMES), np.int32)
    plain = {k: v.clone() for k, v in process_cohort(*ins).items()}
    fn = lambda *a: process_cohort(*a, sweep=True, sweep_route=route, sweep_symbol_rank=rank)   # noqa: E731
    eager = {k: v.clone() for k, v in fn(*ins).items()}
    graph = CapturedPipeline(fn, *other)
    replay = {k: v.clone() for k, v in graph(*ins).items()}
    again = process_cohort(*ins)
    torch.cuda.synchronize()
    # without sweep: the same keys in the same order, the same bits, before and after the sweep calls
    assert list(again) == list(plain) == [k for k in eager if not k.startswith("sweep.")]
    n = int(plain["h1.bins"].max())
    for k in plain:
        for name, got in (("again", again[k]), ("sweep=True", eager[k])):
            x, y = got.cpu().numpy(), plain[k].cpu().numpy()
            if k.startswith("h1.") and x.ndim == 2:
                x, y = x[:, :n], y[:, :n]
            np.testing.assert_array_equal(x, y, err_msg=f"{name} {k}")
    assert sorted(k for k in eager if k.startswith("sweep.")) == [
        "sweep.candidate", "sweep.rank_score", "sweep.status", "sweep.winner", "sweep.winner_score"]
    # the sweep outputs: liquidation_sweep_select on the cohort's own pump.* at column T - 2
    cols = {k: ins[8] if k == "close" else plain[f"pump.{k}"] for k in ref.COLUMNS}
    cols["score_cross"] = plain["pump.score_cross"]
    u = T - 2
    want = signals.liquidation_sweep_select(cols, route_ok=route.reshape(-1, 1).expand(pg.S, T).contiguous(),
                                            symbol_rank=rank)
    for name, got in (("eager", eager), ("graph", replay)):
        for k in ("status", "candidate", "rank_score"):
            np.testing.assert_array_equal(got[f"sweep.{k}"].cpu().numpy(), want[k][:, u].cpu().numpy(),
                                          err_msg=f"{name} {k}")
        for k in ("winner", "winner_score"):
            np.testing.assert_array_equal(got[f"sweep.{k}"].cpu().numpy(), want[k][u:u + 1].cpu().numpy(),
                                          err_msg=f"{name} {k}")
        assert tuple(got["sweep.status"].shape) == (pg.S,) and tuple(got["sweep.winner"].shape) == (1,)
    host_cols = {k: cols[k].cpu().numpy() for k in ref.COLUMNS}
    r = ref.select(host_cols, cols["score_cross"].cpu().numpy(), route_ok=np.repeat(p["route_ok"][:, u:u + 1], T, 1),
                   symbol_rank=ref.symbol_ranks(pg.NAMES))
    assert (eager["sweep.status"].cpu().numpy() == r["status"][:, u]).all()
    assert int(eager["sweep.winner"][0]) == r["winner"][u]
    assert (r["status"][:, u] == 0).sum() >= 1   # the cohort's message has a candidate


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_end_to_end_from_candles(cuda):
    """pump_score_features(exact=True) on the fixture's candles (each row's
    frame starts at its first_t), then the select: equal to the restatement on
    the same device columns, and to the real signal()'s candidates and the
    selector's dispatches at every cell without a near-tie."""
    from binquant_amd import signals, strategies

    fx, p = sc.fixture(), sc.panel()
    S, T = pg.S, pg.T
    keys = [k for k in ref.COLUMNS if k != "close"] + ["score_cross"]
    dev = {k: (torch.zeros((S, T), dtype=torch.bool, device="cuda") if k == "score_cross" else
               torch.full((S, T), float("nan"), dtype=torch.float64, device="cuda")) for k in keys}
    for f in sorted(set(p["first_t"].tolist())):
        rows = np.flatnonzero(p["first_t"] == f)
        o, h, l, c, v = (dv(p[k][rows][:, f:]) for k in ("open", "high", "low", "close", "volume"))
        feats = strategies.pump_score_features(o, h, l, c, v, dv(p["btc_close"][f:]), exact=True)
        for k in keys:
            dev[k][torch.from_numpy(rows).cuda(), f:] = feats[k]
    rank = ref.symbol_ranks(pg.NAMES)
    got = host(signals.liquidation_sweep_select(dev, close=dv(p["close"]), route_ok=dv(p["route_ok"], bool),
                                                first_t=dv(p["first_t"]), lens=dv(p["lens"]),
                                                symbol_rank=dv(rank, np.int32)))
    hcols = {k: (p["close"] if k == "close" else dev[k].cpu().numpy()) for k in ref.COLUMNS}
    want = ref.select(hcols, dev["score_cross"].cpu().numpy(), route_ok=p["route_ok"], first_t=p["first_t"],
                      lens=p["lens"], symbol_rank=rank)
    assert_select_equal(got, want, "device columns")
    fcols, fcross = sc.fixture_columns()
    ties = sc.near_tie_mask(fcols, fcross, first_t=p["first_t"], lens=p["lens"])
    assert ties.sum() == 0
    fwant = ref.select(fcols, fcross, route_ok=p["route_ok"], first_t=p["first_t"], lens=p["lens"], symbol_rank=rank)
    bad = np.argwhere((got["status"] != fwant["status"]) & ~ties)
    report = [(int(s), int(t), int(got["status"][s, t]), int(fwant["status"][s, t]),
               {k: (float(hcols[k][s, t]), float(fcols[k][s, t])) for k in ref.COLUMNS
                if not sc.same_bits(hcols[k][s, t], fcols[k][s, t]).all()}) for s, t in bad[:5]]
    assert len(bad) == 0, f"exact-mode columns decide differently from the reference at {report}"
    assert (got["candidate"] == fx["submitted"]).all()
    assert (got["winner"] == fx["dispatched"]).all()
