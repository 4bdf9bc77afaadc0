"""GradualGainerRetest.signal()'s watchlist replay on the device
(signals.gradual_gainer_retest / engine.retest_replay, bq_retest.hip): against
what the REAL method did candle by candle (tests/golden/retest_gates.npz) and,
at the kernel's step edges, against the numpy restatement that fixture pins
(tests/retest_ref.py). Events, detail bits, levels and states: all exact."""

import numpy as np
import pytest
import torch

from tests import retest_cases as rc
from tests.retest_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    return tuple(x.cpu().numpy() for x in res)


def device_state(state):
    return tuple(dv(np.asarray(x, dt)) for x, dt in zip(state, (np.uint8, np.int64, np.float64)))


def replay(p, risk=True, state=None, rows=slice(None), **kw):
    """engine.retest_replay on numpy inputs; returns (event, detail, level)
    and, with a state, the state after the call."""
    from binquant_amd import engine

    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    st = device_state(state) if state is not None else None
    res = engine.retest_replay(*(dv(p[k][rows]) for k in rc.COLS + ("ema", "open_time", "leader")),
                               dv(p["risk_ok"][rows]) if risk else None, state=st, **kw)
    return host(res), (host(st) if st is not None else None)


def fixture_inputs():
    fx, p = rc.fixture(), rc.panel()
    return {**{k: p[k] for k in rc.COLS + ("open_time", "risk_ok")}, "ema": fx["ema"], "leader": fx["leader"]}


def test_kernel_equals_reference_panel(cuda):
    """All rows in one launch; the carry-out state is the recorded
    strategy_states entry after each row's last candle."""
    fx, p = rc.fixture(), rc.panel()
    idle = (np.zeros(pg.S, np.uint8), np.zeros(pg.S, np.int64), np.full(pg.S, np.nan))
    got, state = replay(fixture_inputs(), state=idle, first_t=p["first_t"], lens=p["lens"], from_t=p["first_t"],
                        **rc.fixture_params())
    rc.assert_replay_equal(got, (fx["event"], fx["detail"], fx["level"]), "panel")
    rc.assert_state_equal(state, rc.recorded_state(p["lens"] - 1), "carry-out")
    stateless, _ = replay(fixture_inputs(), first_t=p["first_t"], lens=p["lens"], from_t=p["first_t"])
    rc.assert_replay_equal(stateless, got, "no state, default parameters")


@pytest.mark.parametrize("split", range(5))
def test_resume_from_recorded_state(cuda, split):
    """From the recorded state after candle k - 1 (k: a seeded split point
    per row, 5 per row in all), candles [k, lens) reproduce the recording."""
    fx, p = rc.fixture(), rc.panel()
    g = np.random.default_rng(100 + split)
    k = g.integers(p["first_t"] + 100, p["lens"])
    got, state = replay(fixture_inputs(), state=rc.recorded_state(k - 1), first_t=p["first_t"], lens=p["lens"],
                        from_t=k, **rc.fixture_params())
    cols = np.arange(pg.T)
    tail = (cols >= k[:, None]) & (cols < p["lens"][:, None])
    for name, x, want in zip(("event", "detail"), got, (fx["event"], fx["detail"])):
        assert (x[tail] == want[tail]).all(), name
        assert (x[~tail] == (ref.RT_NO_FRAME if name == "event" else 0)).all(), name
    assert rc.same_bits(got[2][tail], fx["level"][tail]).all() and np.isnan(got[2][~tail]).all()
    rc.assert_state_equal(state, rc.recorded_state(p["lens"] - 1), f"split {split}")


EDGE_T = (63, 64, 65, 129, 1025, 2049)


@pytest.mark.parametrize("T", EDGE_T)
def test_step_edges_vs_restatement(cuda, T):
    """Watches set in one 64-candle step and resolved, expired or blocked in
    a later one; leaders at lanes 0 and 63; the level's window reaching back
    across the step; lens < T, from_t > 0, risk_ok None, a padded row pitch."""
    from binquant_amd import engine

    p = rc.edge_panel(T, seed=T)
    args = [p[k] for k in rc.COLS + ("ema", "open_time", "leader")]
    want = ref.retest_replay(*args, p["risk_ok"], **rc.EDGE_PARAMS)
    got, _ = replay(p, **rc.EDGE_PARAMS)
    rc.assert_replay_equal(got, want, f"T={T}")
    ev = want[0]
    if T >= 1025:   # the situations the panel is for, counted on the restatement
        step = np.arange(T) // rc.WAVE
        lane = np.arange(T) % rc.WAVE
        assert ((ev == ref.RT_WATCH_SET) & (lane == 0)).sum() >= 3 and ((ev == ref.RT_WATCH_SET) & (lane == 63)).sum() >= 3
        crossed = {ref.RT_CANDIDATE: 0, ref.RT_RISK_BLOCKED: 0, "expired": 0}
        for s in range(rc.EDGE_S):
            set_step = None
            for t in range(T):
                if want[1][s, t] & ref.D_EXPIRED and set_step is not None:
                    crossed["expired"] += step[t] > set_step
                    set_step = None
                if ev[s, t] == ref.RT_WATCH_SET:
                    set_step = step[t]
                elif ev[s, t] in (ref.RT_CANDIDATE, ref.RT_RISK_BLOCKED) and set_step is not None:
                    crossed[ev[s, t]] += step[t] > set_step
                    if ev[s, t] == ref.RT_CANDIDATE:
                        set_step = None
        assert min(crossed.values()) >= 3, crossed
        assert all((ev == k).sum() >= 10 for k in range(6)), np.bincount(ev.ravel(), minlength=6)
    # ragged rows, a late start and a carried-in watch
    g = np.random.default_rng(T)
    lens = g.integers(0, T + 1, rc.EDGE_S)
    lens[0] = T
    from_t = np.minimum(g.integers(0, T, rc.EDGE_S), lens)
    from_t[1] = 0
    first = np.where(g.random(rc.EDGE_S) < 0.5, 0, g.integers(0, max(T - 20, 1), rc.EDGE_S))
    state = (np.array([1, 0, 1, 0, 1, 1], np.uint8), p["open_time"][:, 0] - 5 * rc.STEP, p["high"][:, 0] * 1.001)
    kw = dict(first_t=first, lens=lens, from_t=from_t, **rc.EDGE_PARAMS)
    want2 = ref.retest_replay(*args, p["risk_ok"], state=state, **kw)
    got2, st2 = replay(p, state=state, **kw)
    rc.assert_replay_equal(got2, want2, f"T={T} ragged")
    rc.assert_state_equal(st2, want2[3], f"T={T} ragged")
    # risk_ok None = a mask of ones
    want3 = ref.retest_replay(*args, None, **rc.EDGE_PARAMS)
    got3, _ = replay(p, risk=False, **rc.EDGE_PARAMS)
    rc.assert_replay_equal(got3, want3, f"T={T} no risk mask")
    # a padded row pitch on every input (ld = T + 192), event only
    def padded(a):
        t = dv(a)
        buf = torch.zeros((t.shape[0], T + 192), dtype=t.dtype, device="cuda")
        buf[:, :T] = t
        return buf[:, :T]

    cols = [padded(x) for x in args] + [padded(p["risk_ok"])]
    assert cols[0].stride(0) == T + 192 and cols[6].stride(0) == T + 192
    e4, d4, l4 = engine.retest_replay(*cols, detail=False, level=False, **rc.EDGE_PARAMS)
    assert d4 is None and l4 is None and (e4.cpu().numpy() == want[0]).all()


@pytest.mark.parametrize("T,k", [(129, 63), (129, 64), (129, 65), (1025, 128), (1025, 960), (1025, 1024)])
def test_split_run_equals_whole(cuda, T, k):
    """[0, k) then [k, T) with the carried state, k at and around step edges,
    is bit-equal to the whole run."""
    p = rc.edge_panel(T, seed=1000 + T)
    idle = (np.zeros(rc.EDGE_S, np.uint8), np.zeros(rc.EDGE_S, np.int64), np.full(rc.EDGE_S, np.nan))
    whole, st_whole = replay(p, state=idle, **rc.EDGE_PARAMS)
    head, st_head = replay(p, state=idle, lens=np.full(rc.EDGE_S, k), **rc.EDGE_PARAMS)
    tail, st_tail = replay(p, state=st_head, from_t=np.full(rc.EDGE_S, k), **rc.EDGE_PARAMS)
    rc.assert_replay_equal(head, whole, "head", slice(0, k))
    rc.assert_replay_equal(tail, whole, "tail", slice(k, None))
    assert (head[0][:, k:] == ref.RT_NO_FRAME).all() and (tail[0][:, :k] == ref.RT_NO_FRAME).all()
    rc.assert_state_equal(st_tail, st_whole, "carry-out")
    assert st_head[0].any() and (whole[0] == ref.RT_CANDIDATE).sum() >= 5


def test_long_lookback(cuda):
    """breakout_lookback = 64: the window is the whole previous step."""
    p = rc.edge_panel(321, seed=5)
    kw = dict(min_history=65, breakout_lookback=64, watch_ms=20 * rc.STEP)
    want = ref.retest_replay(*(p[k] for k in rc.COLS + ("ema", "open_time", "leader")), p["risk_ok"], **kw)
    got, _ = replay(p, **kw)
    rc.assert_replay_equal(got, want, "L=64")
    assert (want[0] == ref.RT_WATCH_SET).sum() >= 10


def test_signals_end_to_end(cuda):
    """signals.gradual_gainer_retest with the leadership and the EMA computed
    on the device: the rows whose frame starts at candle 0 in one call, the
    two late rows as their trimmed frames."""
    from binquant_amd import signals

    fx, p = rc.fixture(), rc.panel()
    late = np.zeros(pg.S, bool)
    late[list(pg.FIRST_T)] = True
    groups = [(np.flatnonzero(~late), 0)] + [(np.array([s]), f) for s, f in pg.FIRST_T.items()]
    for rows, f in groups:
        state = signals.RetestState.idle(len(rows), "cuda")
        res = signals.gradual_gainer_retest(*(dv(p[k][rows, f:]) for k in rc.COLS + ("open_time",)),
                                            dv(p["btc_time"]), dv(p["btc_close"]), risk_ok=dv(p["risk_ok"][rows, f:]),
                                            state=state, lens=dv(p["lens"][rows] - f))
        assert list(res) == ["event", "detail", "breakout_level", "leader", "rs_2h", "rs_6h", "ema20"]
        want = tuple(fx[k][rows, f:] for k in ("event", "detail", "level"))
        rc.assert_replay_equal(host((res["event"], res["detail"], res["breakout_level"])), want, f"rows from {f}")
        inside = np.arange(pg.T - f) < (p["lens"][rows] - f)[:, None]
        assert (res["leader"].cpu().numpy()[inside] == fx["leader"][rows, f:][inside]).all()
        want_state = tuple(x[rows] for x in rc.recorded_state(p["lens"] - 1))
        rc.assert_state_equal(host(state.tensors()), want_state, f"state, rows from {f}")


def test_risk_allows_equals_reference(cuda):
    """signals.retest_risk_allows against the real _risk_allows over the
    fixture's stand-in contexts: allowed and the reason, exact."""
    from binquant_amd import _lib, signals

    fx = rc.fixture()
    n = len(fx["risk_ok"])
    code = lambda names, table: np.array([table.index(str(x)) if str(x) else -1 for x in names], np.int8)   # noqa: E731
    row = lambda k: dv(fx[f"risk_in_{k}"].astype(np.float64))   # noqa: E731
    ok, reason = signals.retest_risk_allows(
        row("stress"), row("regime_score"), row("btc_return"), dv(fx["risk_in_context_ok"].astype(bool)),
        row("atr_pct").reshape(1, n), dv(code(fx["risk_in_regime"], _lib.MICRO_REGIMES)).reshape(1, n),
        dv(code(fx["risk_in_transition"], _lib.MICRO_TRANSITIONS)).reshape(1, n), row("trend").reshape(1, n),
        dv(fx["risk_in_features_ok"].astype(bool)).reshape(1, n))
    assert ok.dtype == torch.bool and reason.dtype == torch.uint8 and tuple(ok.shape) == (1, n)
    bad = np.flatnonzero(reason.cpu().numpy()[0] != fx["risk_reason"])
    assert len(bad) == 0, [(int(i), signals.RISK_REASONS[int(reason[0, i])],
                            signals.RISK_REASONS[int(fx["risk_reason"][i])]) for i in bad[:5]]
    assert (ok.cpu().numpy()[0] == fx["risk_ok"]).all()


def test_cohort_retest_candle_by_candle(cuda):
    """process_cohort(retest=state) fed 40 growing prefixes of 8 fixture rows
    equals the panel replay's columns; without a state its outputs are the
    same dict as before."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.synth import numpy_panel

    fx, p = rc.fixture(), rc.panel()
    rows, t_first, n = np.arange(8), 360, 40
    p5 = numpy_panel(len(rows), 400, seed0=3, edges=True)
    five = [dv(p5[k]) for k in ("open", "high", "low", "close", "volume")]

    def inputs(T):
        return five + [dv(p[k][rows, :T]) for k in rc.COLS] + [dv(p5["volume"][:, :T]), dv(p["open_time"][rows, :T]),
                                                               dv(p["btc_time"][:T]), dv(p["btc_close"][:T])]

    state = signals.RetestState(*device_state(tuple(x[rows] for x in rc.recorded_state(np.full(pg.S, t_first - 1)))))
    ev, dt, lv = (np.empty((len(rows), n), d) for d in (np.uint8, np.uint8, np.float64))
    for i in range(n):
        T = t_first + i + 1
        out = process_cohort(*inputs(T), retest=state, retest_risk=dv(p["risk_ok"][rows, T - 1]))
        ev[:, i], dt[:, i], lv[:, i] = (out[f"retest.{k}"].cpu().numpy() for k in ("event", "detail", "breakout_level"))
    cols = slice(t_first, t_first + n)
    rc.assert_replay_equal((ev, dt, lv), tuple(fx[k][rows, cols] for k in ("event", "detail", "level")), "cohort")
    want_state = tuple(x[rows] for x in rc.recorded_state(np.full(pg.S, t_first + n - 1)))
    rc.assert_state_equal(host(state.tensors()), want_state, "cohort state")
    assert len(np.unique(ev)) >= 4
    plain = process_cohort(*inputs(400))
    with_state = process_cohort(*inputs(400), retest=signals.RetestState.idle(len(rows), "cuda"))
    assert not any(k.startswith("retest.") for k in plain)
    assert [k for k in with_state if k not in plain] == ["retest.event", "retest.detail", "retest.breakout_level"]


def test_cohort_retest_captured_graph_carries_state(cuda):
    """The cohort with a watchlist captured as one graph: the state tensors
    are updated in place by every replay (set after the capture, whose
    warm-up calls advance them), and three replayed messages equal three
    eager ones — outputs and state."""
    import functools

    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline
    from binquant_amd.synth import numpy_panel

    p = rc.panel()
    rows, T = np.arange(8), 400
    p5 = numpy_panel(len(rows), T, seed0=3, edges=True)
    five = [dv(p5[k]) for k in ("open", "high", "low", "close", "volume")]

    def inputs(end):   # the 400-candle window ending before `end`
        w = slice(end - T, end)
        return five + [dv(p[k][rows, w]) for k in rc.COLS] + [dv(p5["volume"]), dv(p["open_time"][rows, w]),
                                                              dv(p["btc_time"][w]), dv(p["btc_close"][w])]

    start = tuple(x[rows] for x in rc.recorded_state(np.full(pg.S, 419)))
    eager_state, graph_state = (signals.RetestState(*device_state(start)) for _ in range(2))
    risk = dv(p["risk_ok"][rows, 420])
    graph = CapturedPipeline(functools.partial(process_cohort, retest=graph_state, retest_risk=risk), *inputs(421))
    for dst, src in zip(graph_state.tensors(), device_state(start)):
        dst.copy_(src)
    seen = set()
    for end in (421, 422, 423):
        risk.copy_(dv(p["risk_ok"][rows, end - 1]))
        want = process_cohort(*inputs(end), retest=eager_state, retest_risk=risk)
        got = graph(*inputs(end))
        torch.cuda.synchronize()
        for k in ("event", "detail"):
            assert torch.equal(got[f"retest.{k}"], want[f"retest.{k}"]), (end, k)
        assert rc.same_bits(got["retest.breakout_level"].cpu().numpy(), want["retest.breakout_level"].cpu().numpy()).all()
        rc.assert_state_equal(host(graph_state.tensors()), host(eager_state.tensors()), f"message {end}")
        seen |= set(want["retest.event"].cpu().numpy().tolist())
    assert len(seen) >= 2 and eager_state.active.any()


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    p = rc.edge_panel(130, seed=1)
    good = [dv(p[k]) for k in rc.COLS + ("ema", "open_time", "leader")]
    for kw in (dict(breakout_lookback=0), dict(breakout_lookback=65), dict(breakout_lookback=12, min_history=12)):
        with pytest.raises(ValueError, match="breakout_lookback"):
            engine.retest_replay(*good, **kw)
    for i, bad in ((2, good[2].float()), (3, good[3][:, :-1]), (5, good[5].int()), (6, good[6].to(torch.uint8)),
                   (0, good[0].cpu())):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            engine.retest_replay(*args)
    with pytest.raises(ValueError):
        engine.retest_replay(*good, dv(p["risk_ok"]).cpu())
    with pytest.raises(ValueError):
        engine.retest_replay(*good, state=(dv(np.zeros(6, np.uint8)), dv(np.zeros(6, np.int32)), dv(np.zeros(6))))
