"""GPU: bq_buy_the_dip_replay (bq_dip.hip) and its Python layers against what
the real methods did (tests/golden/dip_gates.npz) and, at the kernel's step
edges, against the numpy restatement that fixture pins (tests/dip_ref.py).
Codes exact; values bit for bit with ema20 given; with the EMA formed in the
pass ema20 at 1e-9 relative (DESIGN §3's bar for in-pass EMAs) and the
point-wise columns (reference_price, change_6h) still bit for bit."""

import functools

import numpy as np
import pytest
import torch

from tests import dip_cases as dc
from tests.dip_cases import pg, ref

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


def replay(p, *, pad=0, ema=None, market="panel", micro="panel", columns=ref.VALUES, **kw):
    """signals.buy_the_dip_entry on numpy inputs; returns replay()'s layout."""
    from binquant_amd import signals

    put = (lambda a: pitched(a, pad)) if pad else dv
    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    market = p["market_regime"] if isinstance(market, str) else market
    micro = p["micro_regime"] if isinstance(micro, str) else micro
    out = signals.buy_the_dip_entry(
        put(p["close"]), dv(p["close_time"]), dv(np.asarray(market, np.int8)) if market is not None else None,
        dv(np.asarray(micro, np.int8)) if micro is not None else None,
        ema20=put(ema) if ema is not None else None, columns=columns, **kw)
    torch.cuda.synchronize()
    assert set(out) == {"status", *columns}
    return {k: v.cpu().numpy() for k, v in out.items()}


def fixture_run(with_ema, **kw):
    fx, p = dc.fixture(), dc.panel()
    return replay(p, ema=fx["ema20"] if with_ema else None, micro=pg.micro_code(p), first_t=p["first_t"],
                  lens=p["lens"], **kw)


def test_fixture_with_recorded_ema_is_bit_exact(cuda):
    want = dc.recorded()
    got = fixture_run(True)
    dc.assert_codes_equal(got, want, "kernel, ema20 given")
    dc.assert_values_bits(got, want, "kernel, ema20 given")
    got = fixture_run(True, pad=7)
    dc.assert_codes_equal(got, want, "kernel, ema20 given, pitched rows")
    dc.assert_values_bits(got, want, "kernel, ema20 given, pitched rows")


def test_fixture_with_in_pass_ema(cuda):
    want = dc.recorded()
    got = fixture_run(False)
    dc.assert_codes_equal(got, want, "kernel, in-pass EMA")
    dc.assert_ema_close(got, want, "kernel, in-pass EMA")
    dc.assert_values_bits(got, want, "point-wise columns", names=dc.POINTWISE)


NAN_AT = [(0, 127), (1, 0), (3, 63), (5, 63), (6, 64), (7, 127), (8, 65), (9, 100), (12, 128)]


def edge_panel(S, T, seed):
    """first_t at 0 / 1 / 63 / 64, lens < T on every fourth row, NaN closes on
    lanes 63 and 0 of a step (rows 1 and 3: before first_t, not in the frame),
    a zero and two infinite closes, gap rows, and rows of 5-minute candles
    with a gap, whose reference lies 72 candles (two steps) back."""
    p = dc.seeded_panel(S, T, seed, nan_at=NAN_AT, gap_rows=(1, 11), dense_rows=(4, 10))
    for s in (4, 10):
        if s < S:
            p["close_time"][s, T // 3:] += 20 * pg.DENSE_STEP_MS
    if S > 2 and T > 94:   # row 2's frame starts at 63: the infinite pair inside it
        p["close"][2, 70] = p["close"][2, 94] = np.inf
    first = np.array([(0, 1, 63, 64, 0)[s % 5] for s in range(S)]).clip(0, max(T - 1, 0))
    lens = np.array([T if s % 4 else max(T - 3, 1) for s in range(S)])
    return p, first, lens


@pytest.mark.parametrize("T", [1, 23, 24, 25, 63, 64, 65, 87, 88, 89, 128, 129, 257])
@pytest.mark.parametrize("S", [1, 5, 70])
def test_step_edges_vs_restatement(cuda, S, T):
    p, first, lens = edge_panel(S, T, seed=2000 + 7 * T + S)
    ema = ref.ema20s(p["close"], first, lens)
    want = dc.ref_replay(p, ema20=ema, first_t=first, lens=lens)
    if S >= 5 and T >= 257:   # what the panel is for
        idx, t = want["reference_index"], np.arange(T)[None, :]
        assert ((idx >= 0) & (idx // 64 <= t // 64 - 2)).any() and ((idx >= 0) & (idx != t - 24))[1].any()
        assert all((want["status"] == c).any() for c in range(8)), np.bincount(want["status"].ravel(), minlength=8)
        assert np.isnan(want["change_6h"][2, 94]) and (want["reference_price"][1] == 0.0).any()
    got = replay(p, pad=7, ema=ema, first_t=first, lens=lens)
    dc.assert_codes_equal(got, want, f"{S}x{T} ema20 given")
    dc.assert_values_bits(got, want, f"{S}x{T} ema20 given")
    got = replay(p, pad=7, first_t=first, lens=lens)
    # a near-tie of close against the EMA could flip a code under the 1e-9 EMA: none in these seeds
    dc.assert_codes_equal(got, want, f"{S}x{T} in-pass EMA")
    dc.assert_values_bits(got, want, f"{S}x{T} in-pass EMA", names=dc.POINTWISE)
    dc.assert_ema_close(got, want, f"{S}x{T} in-pass EMA")


@pytest.mark.parametrize("k", [63, 64, 65])
def test_split_replay_equals_whole(cuda, k):
    S, T = 5, 200
    p, first, _ = edge_panel(S, T, seed=300 + k)
    p["close"][3, k + 30] = np.nan
    for ema in (ref.ema20s(p["close"], first), None):
        whole = replay(p, ema=ema, first_t=first)
        a = replay(p, ema=ema, first_t=first, lens=np.full(S, k))
        b = replay(p, ema=ema, first_t=first, from_t=np.full(S, k))
        for name in ("status",) + ref.VALUES:
            joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
            assert dc.same_bits(joined, whole[name]).all() if name in ref.VALUES else (joined == whole[name]).all(), \
                (name, ema is None)
        assert (b["status"][:, :k] == ref.NO_FRAME).all() and (a["status"][:, k:] == ref.NO_FRAME).all()
        assert (whole["status"][3, k + 30:] == ref.NOT_READY).all()


def test_ema_carry_over_many_steps(cuda):
    """4 x 2049 against pandas' ewm at 1e-9; row 2 holds a mid-frame NaN
    close and is NOT_READY from there on, row 3 an infinite one."""
    S, T = 4, 2049
    p = dc.seeded_panel(S, T, seed=11, specials=False)
    p["close"][2, 1000] = np.nan
    p["close"][3, 5] = np.inf
    first = np.array([0, 70, 0, 0])
    want = dc.ref_replay(p, market_regime=None, micro_regime=None, first_t=first)
    got = replay(p, market=None, micro=None, first_t=first)
    dc.assert_codes_equal(got, want, "long rows")
    dc.assert_values_bits(got, want, "long rows", names=dc.POINTWISE)
    dc.assert_ema_close(got, want, "long rows")
    assert (got["status"][2, 1000:] == ref.NOT_READY).all() and (got["status"][2, 900:1000] != ref.NOT_READY).all()
    reached = ~np.isnan(got["ema20"])
    assert reached[[0, 1, 3], 1500:].sum() > 100 and not reached[2, 1000:].any()


def test_optional_inputs(cuda):
    """One regime for every candle, micro_regime [S], no regimes at all, status alone."""
    S, T = 5, 130
    p, first, lens = edge_panel(S, T, seed=77)
    ema = ref.ema20s(p["close"], first, lens)
    micro = p["micro_regime"][:, 0].copy()
    for code in (2, 0, -1):
        market = np.array([code], np.int8)
        want = dc.ref_replay(p, market_regime=market, micro_regime=micro, ema20=ema, first_t=first, lens=lens)
        got = replay(p, market=market, micro=micro, ema=ema, first_t=first, lens=lens)
        dc.assert_codes_equal(got, want, f"one regime {code}, micro [S]")
        dc.assert_values_bits(got, want, f"one regime {code}, micro [S]")
    assert (want["status"] == ref.EMIT).any() and (want["status"] == ref.NOT_RECLAIMED).any()
    want = dc.ref_replay(p, market_regime=None, micro_regime=None, ema20=ema, first_t=first, lens=lens)
    got = replay(p, market=None, micro=None, ema=ema, first_t=first, lens=lens, columns=())
    dc.assert_codes_equal(got, want, "no regimes, status alone")
    assert not (want["status"] == ref.REGIME_BLOCKED).any()
    got = replay(p, ema=ema, columns=("change_6h",), lookback_candles=30, min_change_pct=-4.0, max_change_pct=-1.0,
                 lookback_ms=3 * 3_600_000, start_time_ms=0)
    want = dc.ref_replay(p, ema20=ema, lookback_candles=30, min_change_pct=-4.0, max_change_pct=-1.0,
                         lookback_ms=3 * 3_600_000, start_time_ms=0)
    dc.assert_codes_equal(got, want, "other params")
    dc.assert_values_bits(got, want, "other params", names=("change_6h",))


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    S, T = 3, 40
    p = dc.seeded_panel(S, T, seed=1)
    c, ct, mk, mr = dv(p["close"]), dv(p["close_time"]), dv(p["market_regime"]), dv(p["micro_regime"])
    engine.buy_the_dip_replay(c, ct, mk, mr)
    for bad in (dict(lookback_candles=1), dict(nope=1), dict(min_change_pct=float("nan")), dict(lookback_ms=0),
                dict(ema_span=0), dict(min_change_pct=-1.0), dict(max_change_pct=float("inf")),
                dict(columns=("nope",)), dict(ema20=c[:, :5]), dict(ema20=c.float()), dict(first_t=[0, 1]),
                dict(lens=torch.ones(S))):
        with pytest.raises(ValueError):
            engine.buy_the_dip_replay(c, ct, mk, mr, **bad)
    for args in ((c.float(), ct, mk, mr), (c[0], ct, mk, mr), (c, ct.int(), mk, mr), (c, ct[:, :5], mk, mr),
                 (c, ct, mk[:5], mr), (c, ct, mk.to(torch.int64), mr), (c, ct, mk, mr[:2]), (c, ct, mk, mr.double()),
                 (c, ct, mk.cpu(), mr), (c, ct, mk, mr.cpu()), (c.t().contiguous().t(), ct, mk, mr)):
        with pytest.raises(ValueError):
            engine.buy_the_dip_replay(*args)


def test_routing_equals_recorded_table(cuda):
    from binquant_amd import signals

    fx, cs = dc.fixture(), pg.routing_cases()
    assert signals.DIP_ROUTE_REASONS == ref.ROUTE_REASONS == tuple(fx["reasons"])
    col = lambda a: dv(np.asarray(a).reshape(-1, 1))   # noqa: E731  ([N, 1]: one case per row)
    auto, reason = signals.buy_the_dip_routing(col(cs["context_ok"]), col(cs["transitioning"]), col(cs["stress"]),
                                               col(cs["market_regime"]), col(cs["features_ok"]),
                                               col(cs["micro_regime"]))
    assert auto.dtype == torch.bool and reason.dtype == torch.uint8
    assert auto.shape == reason.shape == (len(fx["routing_reason"]), 1)
    assert reason.cpu().numpy().ravel().tolist() == fx["routing_reason"].tolist()
    assert auto.cpu().numpy().ravel().tolist() == fx["routing_autotrade"].tolist()
    # the panel's own contexts: [T] context fields against [S, T] features
    p = dc.panel()
    ctx_ok = p["market_kind"] != pg.MARKET_KINDS.index("none")
    feats_ok = np.array(pg.IN_SNAPSHOT)[:, None] & ctx_ok[None, :]
    auto, reason = signals.buy_the_dip_routing(dv(ctx_ok), dv(p["transitioning"]), dv(p["stress"]),
                                               dv(p["market_regime"]), dv(feats_ok), dv(p["micro_regime"]))
    emit = fx["status"] == ref.EMIT
    assert (reason.cpu().numpy()[emit] == fx["route"][emit]).all()
    assert (auto.cpu().numpy()[emit] == fx["autotrade"][emit]).all()


def cohort_inputs(S, T5, T15, seed=3, close15=None):
    """process_cohort's positional inputs and the 15m close_time; close15: the
    15m close, the other 15m prices formed around it."""
    from binquant_amd.synth import numpy_panel

    p5, p15 = numpy_panel(S, T5, seed0=seed, edges=False), numpy_panel(S, T15, seed0=seed + 100, edges=False)
    if close15 is not None:
        opn = np.concatenate([close15[:, :1], close15[:, :-1]], axis=1)
        p15 = dict(p15, open=opn, close=close15, high=np.maximum(opn, close15) * 1.001,
                   low=np.minimum(opn, close15) * 0.999)
    ts15 = np.tile(pg.START_MS + np.arange(T15, dtype=np.int64) * STEP15, (S, 1))
    btc = 60000.0 * np.exp(np.cumsum(np.random.default_rng(5).normal(0.0, 0.001, T15)))
    cols = ("open", "high", "low", "close", "volume")
    args = [dv(p5[k]) for k in cols] + [dv(p15[k]) for k in cols] + [dv(ts15), dv(ts15[0]), dv(btc)]
    return args, ts15 + STEP15 - 1


STEP15 = pg.STEP_MS


def test_cohort_outputs_equal_standalone_calls(cuda):
    """process_cohort(buy_the_dip=True) at 40 x 130 (5m) / 40 x 120 (15m): the
    new outputs equal the stand-alone call on the newest candle; without the
    keyword the dict's keys and values equal a call on the parent's
    signature."""
    from binquant_amd import signals
    from binquant_amd.cohort import process_cohort

    S, T5, T15 = 40, 130, 120
    args, ct15 = cohort_inputs(S, T5, T15)
    rng = np.random.default_rng(8)
    mkt, micro = dv(np.array([2], np.int8)), dv(rng.choice([-1, 0, 1, 2, 3, 4], S).astype(np.int8))
    plain = process_cohort(*args)
    parent_keys = list(plain)
    assert not any(k.startswith("dip.") for k in plain)
    full = process_cohort(*args, buy_the_dip=True, ct15=dv(ct15), dip_regimes=(mkt, micro))
    torch.cuda.synchronize()
    assert [k for k in full if k not in plain] == ["dip.status", "dip.reference_price", "dip.change_6h"]
    assert [k for k in full if k in plain] == parent_keys
    for k in parent_keys:
        a, b = plain[k], full[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        a, b = torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)
        if k.startswith("h1.") and a.dim() == 2:   # bins past a row's count are left unwritten
            written = torch.arange(a.shape[1], device="cuda")[None, :] < plain["h1.bins"][:, None]
            a, b = a * written, b * written
        assert torch.equal(a, b), k
    alone = signals.buy_the_dip_entry(args[8], dv(ct15), mkt, micro)
    for k in ("status", "reference_price", "change_6h"):
        a, b = alone[k][:, -1], full[f"dip.{k}"]
        assert a.shape == b.shape == (S,)
        assert dc.same_bits(a.cpu().numpy(), b.cpu().numpy()).all() if a.dtype == torch.float64 else torch.equal(a, b), k
    want = ref.replay(args[8].cpu().numpy(), ct15, np.array([2]), micro.cpu().numpy())
    assert (full["dip.status"].cpu().numpy() == want["status"][:, -1]).all()
    assert (want["status"][:, -1] >= ref.OUT_OF_BAND).any()
    none = process_cohort(*args, buy_the_dip=True, ct15=dv(ct15))   # no context: nothing blocks
    assert not (none["dip.status"] == ref.REGIME_BLOCKED).any()
    with pytest.raises(ValueError):
        process_cohort(*args, buy_the_dip=True)


def test_cohort_graph_replay_equals_eager(cuda):
    """process_cohort(buy_the_dip=True) captured once and replayed over three
    messages (a window sliding by one candle): ct15 and the regimes are device
    tensors updated in place between replays; dip.* equal eager calls'."""
    from binquant_amd.cohort import process_cohort
    from binquant_amd.graphs import CapturedPipeline

    S, T5, W = 8, 100, 80   # the newest candles 80-82 lie on the pattern's first recovery
    dipp = dc.seeded_panel(S, W + 3, seed=31, specials=False)   # a 15m close dense in dips that reclaim
    full_args, ct_all = cohort_inputs(S, T5, W + 3, seed=9, close15=dipp["close"])
    rng = np.random.default_rng(2)
    micro_all = rng.choice([-1, 0, 2, 4], (S, W + 3)).astype(np.int8)

    def window(e):
        a = list(full_args)
        for i in range(5, 11):   # the 15m panels and ts15
            a[i] = full_args[i][:, e - W:e].contiguous()
        a[11], a[12] = full_args[11][e - W:e].contiguous(), full_args[12][e - W:e].contiguous()
        return a

    ct15, mkt, micro = dv(ct_all[:, :W]), dv(np.array([2], np.int8)), dv(micro_all[:, W - 1])
    fn = functools.partial(process_cohort, buy_the_dip=True, ct15=ct15, dip_regimes=(mkt, micro))
    graph = CapturedPipeline(fn, *window(W))
    seen = []
    for e, code in ((W + 1, 2), (W + 2, 0), (W + 3, -1)):
        ct15.copy_(dv(ct_all[:, e - W:e]))
        mkt.fill_(code)
        micro.copy_(dv(micro_all[:, e - 1]))
        want = {k: v.clone() for k, v in fn(*window(e)).items() if k.startswith("dip.")}
        got = graph(*window(e))
        torch.cuda.synchronize()
        assert set(want) == {"dip.status", "dip.reference_price", "dip.change_6h"}
        for k in want:
            assert dc.same_bits(got[k].double().cpu().numpy(), want[k].double().cpu().numpy()).all(), (e, k)
        alone = ref.replay(dipp["close"][:, e - W:e], ct_all[:, e - W:e], np.array([code]), micro_all[:, e - 1])
        assert (got["dip.status"].cpu().numpy() == alone["status"][:, -1]).all(), e
        seen.append(got["dip.status"].cpu().numpy().copy())
    assert len({s.tobytes() for s in seen}) > 1   # the messages differ
