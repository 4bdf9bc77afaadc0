"""GPU: bq_price_tracker_replay (bq_pricetracker.hip) and its Python layers
against what the real methods did (tests/golden/pricetracker_gates.npz) and,
at the kernel's step edges, against the numpy restatement that fixture pins
(tests/pricetracker_ref.py). Codes, detail bits and cooldown entries exact;
values bit for bit with trend_score given, at 1e-9 with the EMA formed in the
pass (trend_score relative — DESIGN §3's bar for in-pass EMAs — the score
fields absolute: clamped sums with coefficients <= 0.4 on trend_score)."""

import functools

import numpy as np
import pytest
import torch

from tests import pricetracker_cases as pc
from tests.pricetracker_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=7):
    """[S, T] on a row pitch of T + pad."""
    S, T = a.shape
    buf = torch.full((S, T + pad), float("nan") if a.dtype.kind == "f" else 0, dtype=torch.from_numpy(a[:0]).dtype,
                     device="cuda")
    buf[:, :T] = dv(a)
    return buf[:, :T]


def replay(p, *, state=None, pad=0, hlv=True, trend=None, columns=ref.VALUES, **kw):
    """engine.price_tracker_replay on numpy inputs; returns replay()'s layout
    and, with a state, the state after the call."""
    from binquant_amd import engine

    put = (lambda a: pitched(a, pad)) if pad else dv
    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    st = (dv(np.asarray(state[0], np.uint8)), dv(np.asarray(state[1], np.int64))) if state is not None else None
    opt = {k: put(p[n]) for k, n in (("h", "high"), ("l", "low"), ("v", "volume"))} if hlv else {}
    rs = p["symbol_rs"]
    status, detail, vals = engine.price_tracker_replay(
        *(put(p[k]) for k in pc.PANELS), dv(p["close_time"]), put(rs) if rs.ndim == 2 else dv(rs), dv(p["ctx"]),
        dv(np.asarray(p["ctx_ok"], bool).reshape(-1)) if p.get("ctx_ok") is not None else None,
        trend_score=put(trend) if trend is not None else None, state=st, columns=columns, **opt, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in vals.items()}
    out.update(status=status.cpu().numpy(), detail=detail.cpu().numpy())
    return out, (tuple(x.cpu().numpy() for x in st) if st is not None else None)


def fixture_run(with_trend, **kw):
    fx, p = pc.fixture(), pc.panel()
    return replay(p, trend=fx["trend_score"] if with_trend else None, first_t=p["first_t"], lens=p["lens"], **kw)


def test_fixture_with_recorded_trend_is_bit_exact(cuda):
    fx = pc.fixture()
    got, state = fixture_run(True, state=(np.zeros(pg.S), np.zeros(pg.S)))
    want = pc.recorded()
    pc.assert_codes_equal(got, want, "kernel, trend given")
    pc.assert_values_bits(got, want, "kernel, trend given")
    pc.assert_state_equal(state, (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")
    stateless, _ = fixture_run(True, pad=7)
    pc.assert_codes_equal(stateless, want, "kernel, no state, pitched rows")
    pc.assert_values_bits(stateless, want, "kernel, no state, pitched rows")


def test_fixture_with_in_pass_ema(cuda):
    fx = pc.fixture()
    got, state = fixture_run(False, state=(np.zeros(pg.S), np.zeros(pg.S)))
    want = pc.recorded()
    pc.assert_codes_equal(got, want, "kernel, in-pass EMA")
    pc.assert_values_close(got, want, "kernel, in-pass EMA")
    pc.assert_state_equal(state, (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")
    pc.assert_values_bits(got, want, "point-wise columns", names=("local_score",))


def test_fixture_repeated_messages(cuda):
    """The same candle sent twice: COOLDOWN the second time (elapsed 0)."""
    fx, p = pc.fixture(), pc.panel()
    reps = p["repeats"]
    t_of = dict((int(s), int(t)) for s, t in reps)
    rows = sorted(t_of)
    t = np.array([t_of[s] for s in rows])
    sub = {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (pg.S,) else v) for k, v in p.items()}
    state = (fx["state_has"][rows, t], fx["state_last"][rows, t])
    got, after = replay(sub, trend=fx["trend_score"][rows], state=state, first_t=p["first_t"][rows], lens=t + 1,
                        from_t=t)
    order = [rows.index(int(s)) for s, _ in reps]
    assert (got["status"][order, t[order]] == fx["repeat_status"]).all()
    assert (after[1][order] == fx["repeat_last"]).all()
    assert (np.delete(got["status"][0], t[0]) == ref.NO_FRAME).all()


@pytest.mark.parametrize("T", [1, 29, 30, 63, 64, 65, 128, 129, 257])
@pytest.mark.parametrize("S", [1, 5, 70])
def test_step_edges_vs_restatement(cuda, S, T):
    """Seeded panels dense in oversold cells on a row pitch of T + 7: lens <
    T, first_t at 0 / 1 / 63 / 64, a NaN tail landing on lanes 0-3 of a step,
    a gap row; trend given (bits) and formed in the pass (1e-9)."""
    nan_at = [(0, 62, "rsi"), (1, 63, "volume"), (2, 127, "macd"), (3, 64, "high"), (4, 60, "low"), (2, 190, "close")]
    p = pc.seeded_panel(S, T, seed=1000 + 7 * T + S, nan_at=nan_at, gap_rows=(1,) if S > 1 and T > 40 else ())
    first = np.array([(0, 1, 63, 64, 0)[s % 5] for s in range(S)]).clip(0, max(T - 1, 0))
    lens = np.array([T if s % 4 else max(T - 3, 1) for s in range(S)])
    trend = ref.trend_scores(p["close"], first, lens)
    want = pc.ref_replay(p, **pc.replay_kwargs(p, trend_score=trend, first_t=first, lens=lens))
    got, state = replay(p, pad=7, trend=trend, first_t=first, lens=lens, state=(np.zeros(S), np.zeros(S)))
    pc.assert_codes_equal(got, want, f"{S}x{T} trend given")
    pc.assert_values_bits(got, want, f"{S}x{T} trend given")
    pc.assert_state_equal(state, want["state"], f"{S}x{T}")
    got, state = replay(p, pad=7, first_t=first, lens=lens, state=(np.zeros(S), np.zeros(S)))
    # a near-tie of a score against its threshold could flip a code under the 1e-9 EMA: none in these seeds
    pc.assert_codes_equal(got, want, f"{S}x{T} in-pass EMA")
    pc.assert_values_close(got, want, f"{S}x{T} in-pass EMA")
    pc.assert_state_equal(state, want["state"], f"{S}x{T} in-pass EMA")


def test_optional_inputs(cuda):
    """high / low / volume absent, symbol_rs [S], one context for every
    candle, ctx_ok absent, status alone."""
    S, T = 5, 130
    p = pc.seeded_panel(S, T, seed=77, per_candle_ctx=False, nan_at=[(0, 70, "volume"), (1, 64, "rsi")])
    p["symbol_rs"] = p["symbol_rs"][:, 0].copy()
    p["ctx"][0] = 0.8
    trend = ref.trend_scores(p["close"])
    q = dict(p, ctx_ok=None)
    want = pc.ref_replay(q, symbol_rs=q["symbol_rs"], ctx=q["ctx"], trend_score=trend)   # no high / low / volume
    got, _ = replay(q, hlv=False, trend=trend)
    pc.assert_codes_equal(got, want, "no h/l/v")
    pc.assert_values_bits(got, want, "no h/l/v")
    assert (want["status"][0, 70:75] != ref.NOT_READY).any() and (want["status"][1, 64:69] == ref.NOT_READY).all()
    p["ctx_ok"] = np.array([False])
    want = pc.ref_replay(p, **pc.replay_kwargs(p, trend_score=trend))
    got, _ = replay(p, trend=trend, columns=())
    pc.assert_codes_equal(got, want, "no context")
    assert (want["status"] == ref.NO_CONTEXT).any() and not (want["status"] == ref.EMIT).any()


def test_cooldown_rules(cuda):
    """One row, every candle past min_history a passing candidate: a window
    spanning the step edge, cooldown_ms = 0, a gap row, a carried-in last
    later than the candle, the same candle twice."""
    T = 100
    p = pc.seeded_panel(2, T, seed=5, setup_rate=1.0, per_candle_ctx=False, gap_rows=(1,))
    p["ctx"][:, 0] = (0.9, 0.4, 0.3, 0.1)
    p["ctx_ok"][:] = True
    p["symbol_rs"][:] = 0.02
    trend = np.zeros((2, T))
    kw = dict(trend=trend, hlv=False)
    got, st = replay(p, state=(np.zeros(2), np.zeros(2)), **kw)
    emits = [np.nonzero(got["status"][s] == ref.EMIT)[0].tolist() for s in range(2)]
    assert emits[0] == [29, 41, 53, 65, 77, 89], emits[0]       # 12 bars apart; 53 -> 65 spans the step edge
    assert (got["status"][0, 54:65] == ref.COOLDOWN).all()
    assert emits[1] == [29, 41, 50, 62, 74, 86, 98], emits[1]  # the 9-bar gap at 50 ends the window sooner
    assert st[1].tolist() == [p["close_time"][0, 89], p["close_time"][1, 98]]
    got, st = replay(p, state=(np.zeros(2), np.zeros(2)), cooldown_ms=0, **kw)
    assert (got["status"][:, 29:] == ref.EMIT).all() and st[0].tolist() == [0, 0]   # strategy_cooldowns is None
    # a carried-in last later than the candle does not block, and is overwritten
    late = p["close_time"][:, 40] + 5 * pc.STEP
    got, st = replay(p, state=(np.ones(2), late), from_t=[35, 35], lens=[40, 40], **kw)
    assert (got["status"][:, 35] == ref.EMIT).all() and st[1].tolist() == p["close_time"][:, 35].tolist()
    assert (got["status"][:, 36:40] == ref.COOLDOWN).all()
    # the same candle twice: elapsed 0
    got, st2 = replay(p, state=st, from_t=[35, 35], lens=[36, 36], **kw)
    assert (got["status"][:, 35] == ref.COOLDOWN).all() and st2[1].tolist() == st[1].tolist()
    want = pc.ref_replay(p, **pc.replay_kwargs(p, trend_score=trend, high=None, low=None, volume=None))
    got, _ = replay(p, **kw)
    pc.assert_codes_equal(got, want, "cooldown panel")


@pytest.mark.parametrize("k", [63, 64, 65])
def test_split_replay_equals_whole(cuda, k):
    S, T = 5, 200
    p = pc.seeded_panel(S, T, seed=300 + k, nan_at=[(0, k - 2, "rsi"), (1, k, "volume"), (3, 20, "close")])
    first = np.array([0, 1, 63, 64, 0])
    for trend in (ref.trend_scores(p["close"], first), None):
        whole, end = replay(p, trend=trend, first_t=first, state=(np.zeros(S), np.zeros(S)))
        a, mid = replay(p, trend=trend, first_t=first, lens=np.full(S, k), state=(np.zeros(S), np.zeros(S)))
        b, fin = replay(p, trend=trend, first_t=first, from_t=np.full(S, k), state=mid)
        for name in ("status", "detail") + ref.VALUES:
            joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
            assert pc.same_bits(joined, whole[name]).all() if name in ref.VALUES else (joined == whole[name]).all(), \
                (name, trend is None)
        assert (b["status"][:, :k] == ref.NO_FRAME).all() and (a["status"][:, k:] == ref.NO_FRAME).all()
        pc.assert_state_equal(fin, end, "split")


def test_state_clone_is_unaffected(cuda):
    from binquant_amd import signals

    p = pc.seeded_panel(3, 80, seed=9)
    state = signals.PriceTrackerState.empty(3, "cuda")
    copy = state.clone()
    args = [dv(p[k]) for k in pc.PANELS] + [dv(p["close_time"]), dv(p["symbol_rs"]), dv(p["ctx"]), dv(p["ctx_ok"])]
    out = signals.price_tracker_entry(*args, state=state)
    torch.cuda.synchronize()
    assert (out["status"] == ref.EMIT).any() and state.has.any()
    assert not copy.has.any() and not copy.last_close_time.any()
    assert set(out) == {"status", "detail", *ref.VALUES}


def test_ema_carry_over_many_steps(cuda):
    """4 x 2049 against pandas' ewm at 1e-9; row 2 holds a mid-frame NaN close."""
    S, T = 4, 2049
    p = pc.seeded_panel(S, T, seed=11, setup_rate=1.0, per_candle_ctx=False)
    p["close"][2, 1000] = np.nan
    p["close"][3, 5] = np.inf
    p["ctx"][:, 0] = (0.9, 0.4, 0.3, 0.1)
    p["ctx_ok"][:] = True
    first = np.array([0, 70, 0, 0])
    got, _ = replay(p, first_t=first, cooldown_ms=0)
    want = ref.trend_scores(p["close"], first)
    m = ~np.isnan(got["trend_score"])
    assert m[:, 100:].sum() > 0.9 * S * (T - 100)
    err = np.abs(got["trend_score"][m] - want[m])
    assert (err <= 1e-9 * np.abs(want[m])).all(), err.max()


def test_python_wrappers_equal_fixture(cuda):
    from binquant_amd import signals
    from tests.test_pricetracker_ref import burst_inputs

    fx = pc.fixture()
    assert signals.PT_ROUTE_REASONS == ref.ROUTE_REASONS
    cs = pg.routing_cases()
    col = lambda a: dv(np.asarray(a).reshape(-1, 1))   # noqa: E731  ([N, 1]: one case per row)
    ok, reason = signals.price_tracker_routing(
        col(cs["context_ok"]), col(cs["transitioning"]), col(cs["stress"]), col(cs["advancers_ratio"]),
        col(cs["long_tailwind"]), col(cs["short_tailwind"]), col(cs["market_regime"]), col(cs["features_ok"]),
        col(cs["micro_regime"]), col(cs["micro_transition"]), col(cs["rs"]), col(cs["trend"]))
    assert reason.cpu().numpy().ravel().tolist() == fx["routing_reason"].tolist()
    assert (ok.cpu().numpy().ravel() == (fx["routing_reason"] == ref.ROUTE_OK)).all()
    ac = pg.autotrade_cases()
    ok, reason = signals.long_autotrade_allows(
        col(ac["context_ok"]), col(ac["transitioning"]), col(ac["timestamp"]), col(ac["stable_since"]),
        col(ac["market_regime"]), col(ac["stress"]), col(ac["features_ok"]), col(ac["micro_regime"]),
        col(ac["micro_transition"]))
    assert ok.cpu().numpy().ravel().tolist() == fx["autotrade_allowed"].tolist()
    assert ((reason.cpu().numpy().ravel() == 0) == fx["autotrade_allowed"]).all()
    q, route, ctx_ok, first = burst_inputs()
    be = signals.activity_burst_entry(dv(q), dv(route), dv(ctx_ok), first_t=dv(first))
    status, autotrade = be["status"].cpu().numpy(), be["autotrade"].cpu().numpy()
    want_status, want_auto = ref.burst_entry(q, route, ctx_ok, first_t=first)
    assert (status == want_status).all() and (autotrade == want_auto).all()
    assert ((status == 0) == fx["burst_emitted"]).all() and (autotrade == fx["burst_autotrade"]).all()


def cohort_inputs(S, T5, T15, seed=3):
    from binquant_amd.synth import numpy_panel

    p5, p15 = numpy_panel(S, T5, seed0=seed, edges=False), numpy_panel(S, T15, seed0=seed + 100, edges=False)
    ts15 = np.tile(pg.T0_MS + np.arange(T15, dtype=np.int64) * 900_000, (S, 1))
    btc = 60000.0 * np.exp(np.cumsum(np.random.default_rng(5).normal(0.0, 0.001, T15)))
    cols = ("open", "high", "low", "close", "volume")
    args = [dv(p5[k]) for k in cols] + [dv(p15[k]) for k in cols] + [dv(ts15), dv(ts15[0]), dv(btc)]
    ct5 = np.tile(pg.T0_MS + (np.arange(T5, dtype=np.int64) + 1) * pc.STEP - 1, (S, 1))
    return args, ct5


def test_cohort_outputs_equal_standalone_calls(cuda):
    """process_cohort(price_tracker=, burst_entry=True) at 40 x 130 (5m) /
    40 x 120 (15m): the new outputs equal the stand-alone calls on the
    cohort's own e5.* / burst.* columns; without the keywords the dict's keys
    and values equal a call on the parent's signature."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort

    S, T5, T15 = 40, 130, 120
    args, ct5 = cohort_inputs(S, T5, T15)
    rng = np.random.default_rng(8)
    ctx, ctx_ok = dv(np.array([[0.9], [0.4], [0.3], [0.1]])), dv(np.array([True]))
    rs, route = dv(rng.normal(0.01, 0.02, S)), dv(rng.random(S) < 0.7)
    plain = process_cohort(*args)
    parent_keys = list(plain)
    assert not any(k.startswith("pricetracker.") or k in ("burst.entry_status", "burst.autotrade") for k in plain)
    state = signals.PriceTrackerState.empty(S, "cuda")
    full = process_cohort(*args, price_tracker=state, ct5=dv(ct5), price_tracker_ctx=(ctx, ctx_ok),
                          price_tracker_rs=rs, burst_entry=True, burst_route=route)
    torch.cuda.synchronize()
    new = [k for k in full if k not in plain]
    assert new == ["pricetracker.status", "pricetracker.detail", "pricetracker.local_score",
                   "pricetracker.adjusted_score", "burst.entry_status", "burst.autotrade"], new
    assert [k for k in full if k in plain] == parent_keys
    assert torch.equal(plain["h1.bins"], full["h1.bins"])
    for k in parent_keys:
        a, b = plain[k], full[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        a, b = torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)
        if k.startswith("h1.") and a.dim() == 2:   # bins past a row's count are left unwritten
            written = torch.arange(a.shape[1], device="cuda")[None, :] < plain["h1.bins"][:, None]
            a, b = a * written, b * written
        assert torch.equal(a, b), k
    newest = torch.full((S,), T5 - 1, dtype=torch.int64, device="cuda")
    alone = signals.price_tracker_entry(args[3], full["e5.rsi"], full["e5.macd"], full["e5.mfi"], dv(ct5), rs, ctx,
                                        ctx_ok, h=args[1], l=args[2], v=args[4],
                                        state=signals.PriceTrackerState.empty(S, "cuda"), from_t=newest)
    for k in ("status", "detail", "local_score", "adjusted_score"):
        a, b = alone[k][:, -1], full[f"pricetracker.{k}"]
        assert a.shape == b.shape == (S,)
        assert pc.same_bits(a.cpu().numpy(), b.cpu().numpy()).all() if a.dtype == torch.float64 else torch.equal(a, b), k
    be = signals.activity_burst_entry(full["burst.qualified_signal"], route.reshape(S, 1), ctx_ok)
    assert torch.equal(be["status"][:, -1], full["burst.entry_status"])
    assert torch.equal(be["autotrade"][:, -1], full["burst.autotrade"])
    none = process_cohort(*args, burst_entry=True)   # no context: nothing is routed, no autotrade
    assert not none["burst.autotrade"].any()
    assert ((none["burst.entry_status"] == signals.AB_EMIT) == full["burst.qualified_signal"][:, -1]).all()


def test_captured_graph_carries_last(cuda):
    """signals.price_tracker_entry on the newest candle captured as one graph
    and replayed over three messages (a window sliding by one candle): the
    state tensors are updated in place by every replay and equal an eager
    run's; the context is updated in place between replays."""
    from binquant_amd import signals
    from binquant_amd.graphs import CapturedPipeline

    S, W = 6, 70
    p = pc.seeded_panel(S, W + 3, seed=21, setup_rate=1.0)
    p["ctx"][:] = np.array([[0.9], [0.4], [0.3], [0.1]])
    p["ctx_ok"][:] = True
    p["ctx_ok"][W] = False   # the second message (newest candle W) has no context
    names = pc.PANELS + ("close_time", "symbol_rs", "high", "low", "volume")
    window = lambda e: [dv(p[k][:, e - W:e]) for k in names]   # noqa: E731
    ctx, ctx_ok = dv(np.ascontiguousarray(p["ctx"][:, W - 1:W])), dv(p["ctx_ok"][W - 1:W])
    newest = torch.full((S,), W - 1, dtype=torch.int64, device="cuda")

    def step(state, c, rsi, macd, mfi, ct, rs, h, l, v):
        out = signals.price_tracker_entry(c, rsi, macd, mfi, ct, rs, ctx, ctx_ok, h=h, l=l, v=v, state=state,
                                          from_t=newest, columns=("adjusted_score",))
        return {k: x[:, -1] for k, x in out.items()}

    eager_state, graph_state = (signals.PriceTrackerState.empty(S, "cuda") for _ in range(2))
    graph = CapturedPipeline(functools.partial(step, graph_state), *window(W))
    for x in graph_state.tensors():
        x.zero_()   # the capture's warm-up calls advanced it
    seen = []
    for e in (W, W + 1, W + 2, W + 3):
        ctx.copy_(dv(np.ascontiguousarray(p["ctx"][:, e - 1:e])))
        ctx_ok.copy_(dv(p["ctx_ok"][e - 1:e]))
        want = {k: x.clone() for k, x in step(eager_state, *window(e)).items()}
        got = graph(*window(e))
        torch.cuda.synchronize()
        for k in want:
            assert pc.same_bits(got[k].double().cpu().numpy(), want[k].double().cpu().numpy()).all(), (e, k)
        pc.assert_state_equal(tuple(x.cpu().numpy() for x in graph_state.tensors()),
                              tuple(x.cpu().numpy() for x in eager_state.tensors()), f"message {e}")
        seen.append(got["status"].cpu().numpy().copy())
    assert (seen[0] == ref.EMIT).all() and (seen[1] == ref.NO_CONTEXT).all() and (seen[2] == ref.COOLDOWN).all()
    assert (graph_state.last_close_time.cpu().numpy() == p["close_time"][:, W - 1]).all()


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    p = pc.seeded_panel(3, 40, seed=1)
    a = [dv(p[k]) for k in pc.PANELS] + [dv(p["close_time"]), dv(p["symbol_rs"]), dv(p["ctx"]), dv(p["ctx_ok"])]
    for bad in (dict(tail_rows=0), dict(nope=1), dict(rsi_max=float("nan")), dict(cooldown_ms=-1),
                dict(columns=("nope",)), dict(state=(a[7], a[4][:, 0])), dict(trend_score=a[0][:, :5]),
                dict(h=a[0].float())):
        with pytest.raises(ValueError):
            engine.price_tracker_replay(*a, **bad)
    with pytest.raises(ValueError):
        engine.price_tracker_replay(*a[:6], dv(p["ctx"][:3]), a[7])
    with pytest.raises(ValueError):
        engine.price_tracker_replay(*a[:4], a[4].int(), *a[5:])
