"""GPU: bq_range_fade_replay (bq_rangefade.hip) and its Python layers against
what the real method did (tests/golden/rangefade_gates.npz) and, at the
kernel's step edges, against the numpy / pandas restatement that fixture pins
(tests/rangefade_ref.py). Codes exact; values bit for bit with the features
given; with the features formed in the pass adx and score within 1e-9 relative
(adx with bq_adx's absolute term at scale 100, test_signals_gpu.py), zscore
within 1e-9 or arbitrated by the exactly computed value on at most 8 cells
(rangefade_cases.assert_values_close), direction bit for bit."""

import numpy as np
import pytest
import torch

from tests import rangefade_cases as rc
from tests.rangefade_cases import pg, ref

pytestmark = pytest.mark.gpu


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pitched(a, pad=7):
    """[S, T] on a row pitch of T + pad."""
    S, T = a.shape
    buf = torch.full((S, T + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = dv(a)
    return buf[:, :T]


def sym_tensors(sym):
    if sym is None:
        return None
    return {"ok": dv(np.asarray(sym["ok"], bool)), "micro_regime": dv(np.asarray(sym["micro_regime"], np.uint8)),
            "micro_transition": dv(np.asarray(sym["micro_transition"], np.uint8)),
            "atr_pct": dv(np.asarray(sym["atr_pct"], np.float64)), "bb_width": dv(np.asarray(sym["bb_width"], np.float64))}


def replay(p, *, pad=0, features=None, columns=ref.VALUES, ctx=None, **kw):
    """signals.range_fade_entry on numpy inputs; returns replay()'s layout."""
    from binquant_amd import signals

    put = (lambda a: pitched(a, pad)) if pad else dv
    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    ft = {k: put(features[k]) for k in ref.FEATURES} if features is not None else None
    ctx_ok = p.get("ctx_ok")
    out = signals.range_fade_entry(
        *(put(p[k]) for k in rc.PANELS), dv(p["ctx"]) if ctx is None else ctx,
        dv(np.asarray(ctx_ok, bool).reshape(-1)) if ctx_ok is not None else None, sym=sym_tensors(p.get("sym")),
        features=ft, columns=columns, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def fixture_inputs():
    p = dict(rc.panel())
    p["sym"] = pg.sym_of(p)
    return p


def test_fixture_with_recorded_features_is_bit_exact(cuda):
    p = fixture_inputs()
    want = rc.recorded()
    got = replay(p, features=rc.recorded_features(), first_t=p["first_t"], lens=p["lens"])
    rc.assert_codes_equal(got, want, "kernel, features given")
    rc.assert_values_bits(got, want, "kernel, features given")


def test_fixture_with_features_formed_in_the_pass(cuda):
    p = fixture_inputs()
    want = rc.recorded()
    got = replay(p, first_t=p["first_t"], lens=p["lens"])
    rc.assert_codes_equal(got, want, "kernel, in-pass features")   # the generator guarantees no near-ties
    rc.assert_values_close(got, want, p["close"], "kernel, in-pass features")


def test_in_pass_features_equal_the_helpers(cuda):
    """first_t = 0, no NaN: adx and zscore, wherever written, equal
    signals.adx(exact=True) and signals.zscore(exact=True) to the same bars."""
    from binquant_amd import signals
    from oracle.indicators_ref import exact_zscore
    from tests.util import assert_close, assert_close_or_exact

    S, T = 6, 200
    p = rc.seeded_panel(S, T, seed=31)
    got = replay(p)
    h, l, c = (dv(p[k]) for k in ("high", "low", "close"))
    adx = signals.adx(h, l, c, exact=True).cpu().numpy()
    z = signals.zscore(c, exact=True).cpu().numpy()
    wa, wz = ~np.isnan(got["adx"]), ~np.isnan(got["zscore"])
    assert wa.sum() >= 200 and wz.sum() >= 100 and (got["status"] == ref.EMIT).sum() >= 5
    assert_close(got["adx"][wa], adx[wa], "adx vs signals.adx(exact=True)", rtol=1e-9, scale=100.0)
    assert_close_or_exact(np.where(wz, got["zscore"], z), z, p["close"], 20, exact_zscore,
                          "zscore vs signals.zscore(exact=True)", max_cases=rc.ZSCORE_MAX_CASES)


NANS = [("close", 0, 62), ("close", 1, 63), ("close", 2, 64), ("close", 0, 20), ("high", 1, 30), ("low", 2, 100),
        ("volume", 0, 63), ("volume", 1, 64), ("rsi", 2, 61), ("rsi", 0, 127), ("open", 1, 126)]


def check_edges(p, what, given_seed=0, **kw):
    """In-pass features to the bars and given features bit for bit, against the restatement."""
    want = rc.ref_replay(p, **kw)
    rc.no_near_ties(want, **{k: v for k, v in kw.items() if k in ref.DEFAULTS})
    got = replay(p, pad=7, **kw)
    rc.assert_codes_equal(got, want, f"{what} in-pass features")
    rc.assert_values_close(got, want, p["close"], f"{what} in-pass features")
    rng = np.random.default_rng(given_seed)
    S, T = p["close"].shape
    ft = {"adx": rng.uniform(5.0, 45.0, (S, T)), "zscore": rng.choice([-1.0, 1.0], (S, T)) * rng.uniform(1.2, 3.6, (S, T))}
    given = rc.ref_replay(p, features_given=ft, **kw)
    got = replay(p, pad=7, features=ft, **kw)
    rc.assert_codes_equal(got, given, f"{what} features given")
    rc.assert_values_bits(got, given, f"{what} features given")
    return want


@pytest.mark.parametrize("T", [1, 39, 40, 64, 65, 103, 129])
@pytest.mark.parametrize("S", [1, 3])
def test_step_edges_vs_restatement(cuda, S, T):
    """Seeded panels dense in setups on a row pitch of T + 7: first_t cycling
    through 0 / 1 / 63, lens < T on some rows, NaN closes at lanes 62 / 63 / 0
    of a step, NaN volume / rsi / open at the last candles of a step (the
    tail(5) of the next step's first lanes), a candle without a range, a
    context per candle with holes, the snapshot [S, T]."""
    first = np.array([(0, 1, 63)[s % 3] for s in range(S)]).clip(0, max(T - 1, 0))
    p = rc.seeded_panel(S, T, seed=4000 + 7 * T + S, first_t=first, nans=NANS)
    lens = np.array([T if s % 2 == 0 else max(T - 3, 1) for s in range(S)])
    want = check_edges(p, f"{S}x{T}", given_seed=T + S, first_t=first, lens=lens)
    if T >= 103:
        assert (want["status"] == ref.EMIT).sum() >= 2 and (want["status"] == ref.NOT_ENOUGH_DATA).sum() >= 40


def test_late_first_candle_and_empty_rows(cuda):
    """first_t = 64 with T = 103: the frame's last candle is its 39th row, one
    short of min_candles, so every candle of the frame is not_enough_data;
    first_t = 63: the first eligible candle (the 40th row) is the last one.
    lens = 0: no frame at all."""
    S, T = 3, 103
    first = np.array([64, 63, 0])
    p = rc.seeded_panel(S, T, seed=11, first_t=first)
    p["ctx"][:, T - 1], p["ctx_ok"][T - 1] = (0.0, 0.1, ref.RANGE), True
    want = check_edges(p, "first_t 64", first_t=first)
    assert (want["status"][0, :64] == ref.NO_FRAME).all() and (want["status"][0, 64:] == ref.NOT_ENOUGH_DATA).all()
    assert (want["status"][1, 63:T - 1] == ref.NOT_ENOUGH_DATA).all() and want["status"][1, T - 1] >= ref.NO_SYMBOL
    lens = np.array([0, T, 0])
    got = replay(p, first_t=first, lens=lens)
    rc.assert_codes_equal(got, rc.ref_replay(p, first_t=first, lens=lens), "lens 0")
    assert (got["status"][[0, 2]] == ref.NO_FRAME).all() and all(np.isnan(got[k][[0, 2]]).all() for k in ref.VALUES)


@pytest.mark.parametrize("k", [63, 64, 100, 130])
def test_from_t_does_not_touch_the_features(cuda, k):
    """from_t > first_t: status 1 before it, and every later column bit for
    bit what the whole replay gives (the features still start at first_t; 130:
    the kernel forms them from the step before from_t's, candle 64, only)."""
    S, T = 3, 150
    first = np.array([0, 1, 45])
    p = rc.seeded_panel(S, T, seed=300 + k, first_t=first, nans=[("close", 1, k - 1), ("rsi", 2, k - 2)])
    whole = replay(p, first_t=first)
    part = replay(p, first_t=first, from_t=np.full(S, k))
    assert (part["status"][:, :k] == ref.NO_FRAME).all() and (part["status"][:, k:] == whole["status"][:, k:]).all()
    for name in ref.VALUES:
        assert np.isnan(part[name][:, :k]).all()
        assert rc.same_bits(part[name][:, k:], whole[name][:, k:]).all(), name
    rc.assert_codes_equal(part, rc.ref_replay(p, first_t=first, from_t=np.full(S, k)), "from_t")
    assert (whole["status"][:, k:] == ref.EMIT).sum() >= 3


def test_a_step_without_a_routed_candle_keeps_the_carried_series(cuda):
    """Candles 64 .. 127 under a TREND_UP market: no candle of that step gets
    as far as the ADX cut, so the kernel leaves its window walks out; the next
    step's windows still read that step's candles."""
    S, T = 3, 200
    p = rc.seeded_panel(S, T, seed=63)
    p["ctx"][2, 64:128] = 0.0
    p["ctx"][:, 128:150], p["ctx_ok"][128:150] = np.array([[0.0], [0.1], [ref.RANGE]]), True
    want = rc.ref_replay(p)
    rc.no_near_ties(want)
    got = replay(p)
    rc.assert_codes_equal(got, want, "unrouted step")
    rc.assert_values_close(got, want, p["close"], "unrouted step")
    assert np.isin(want["status"][:, 64:128], (ref.NO_CONTEXT, ref.TRANSITIONING, ref.STRESS, ref.REGIME_NOT_RANGE)).all()
    reached = ~np.isnan(want["adx"][:, 128:150])
    assert reached.sum() >= 30 and (want["status"][:, 128:150] == ref.EMIT).sum() >= 3


def test_non_contiguous_context(cuda):
    S, T = 3, 129
    p = rc.seeded_panel(S, T, seed=21)
    wide = torch.zeros((3, 2 * T), dtype=torch.float64, device="cuda")
    wide[:, ::2] = dv(p["ctx"])
    got = replay(p, pad=5, ctx=wide[:, ::2])
    want = rc.ref_replay(p)
    rc.assert_codes_equal(got, want, "strided ctx")
    rc.assert_values_close(got, want, p["close"], "strided ctx")


def test_short_min_candles_reaches_the_adx_warm_up(cuda):
    """min_candles = 5 < adx_window = 14: adx is 100 while the frame is shorter
    than the window (adx_too_high), then the zero-filled warm-up mean."""
    S, T = 3, 80
    first = np.array([0, 3, 60])
    p = rc.seeded_panel(S, T, seed=8, first_t=first, per_candle_ctx=False, sym_dims=1)
    want = check_edges(p, "min_candles 5", first_t=first, min_candles=5)
    for s, f in enumerate(first):
        assert (want["adx"][s, f + 4:f + 13] == 100.0).all() and (want["status"][s, f + 4:f + 13] == ref.ADX_TOO_HIGH).all()
        assert (want["adx"][s, f + 13] < 100.0 / 14 + 1e-9) and want["status"][s, f + 13] == ref.NO_SETUP
        assert want["zscore"][s, f + 13] == 0.0   # the z-score's own warm-up


def test_optional_inputs(cuda):
    """sym [S] against [S, T] and ctx [3, 1] against [3, T], identical when
    constant; sym=None; ctx_ok absent and False."""
    S, T = 3, 129
    p = rc.seeded_panel(S, T, seed=77, per_candle_ctx=False, sym_dims=1, nans=[("volume", 0, 70)])
    base = replay(p)
    rc.assert_codes_equal(base, rc.ref_replay(p), "sym [S], ctx [3, 1]")
    assert (base["status"] == ref.EMIT).sum() >= 5
    wide = dict(p, ctx=np.repeat(p["ctx"], T, axis=1), ctx_ok=np.repeat(p["ctx_ok"], T),
                sym={k: np.repeat(v[:, None], T, axis=1) for k, v in p["sym"].items()})
    got = replay(wide)
    for name in ("status",) + ref.VALUES:
        assert rc.same_bits(got[name], base[name]).all() if name != "status" else (got[name] == base[name]).all(), name
    got = replay(dict(p, ctx_ok=None))
    assert (got["status"] == base["status"]).all()
    got = replay(dict(p, sym=None))
    rc.assert_codes_equal(got, rc.ref_replay(dict(p, sym=None)), "sym=None")
    assert np.isin(got["status"], (ref.NO_FRAME, ref.NOT_ENOUGH_DATA, ref.NO_SYMBOL)).all()
    got = replay(dict(p, ctx_ok=np.array([False])), columns=())
    assert set(got) == {"status"}
    assert np.isin(got["status"], (ref.NOT_ENOUGH_DATA, ref.NO_CONTEXT)).all() and (got["status"] == ref.NO_CONTEXT).any()


def test_rows_are_independent(cuda):
    """Any row replayed alone equals the same row in the panel, bit for bit
    (five rows share one workgroup's four waves and the next one's first)."""
    S, T = 5, 150
    first = np.array([0, 1, 63, 64, 20])
    p = rc.seeded_panel(S, T, seed=55, first_t=first, nans=NANS)
    whole = replay(p, first_t=first)
    for s in range(S):
        one = {k: (v[s:s + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (S,) and k not in ("ctx", "ctx_ok") else v)
               for k, v in p.items()}
        one["sym"] = {k: v[s:s + 1] for k, v in p["sym"].items()}
        got = replay(one, first_t=first[s:s + 1])
        assert (got["status"][0] == whole["status"][s]).all(), s
        for name in ref.VALUES:
            assert rc.same_bits(got[name][0], whole[name][s]).all(), (s, name)


@pytest.mark.parametrize("given", [False, True], ids=["in_pass", "given"])
def test_column_subsets(cuda, given):
    """columns=() gives the same status; every subset equals the full run's columns."""
    import itertools

    S, T = 3, 129
    p = rc.seeded_panel(S, T, seed=91)
    ft = {"adx": np.full((S, T), 20.0), "zscore": np.where(p["close"] > p["bb_mid"], 2.5, -2.5)} if given else None
    full = replay(p, features=ft)
    assert (full["status"] == ref.EMIT).sum() >= 5
    for n in range(len(ref.VALUES)):
        for cols in itertools.combinations(ref.VALUES, n):
            got = replay(p, features=ft, columns=cols)
            assert set(got) == {"status", *cols}
            assert (got["status"] == full["status"]).all(), cols
            for name in cols:
                assert rc.same_bits(got[name], full[name]).all(), (cols, name)


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    p = rc.seeded_panel(3, 40, seed=1)
    a = [dv(p[k]) for k in rc.PANELS] + [dv(p["ctx"]), dv(p["ctx_ok"])]
    for bad in (dict(adx_window=0), dict(nope=1), dict(adx_max=float("nan")), dict(zscore_window=65),
                dict(columns=("nope",)), dict(features=(a[0],)), dict(features=(a[0][:, :5],) * 2),
                dict(sym=(a[10],) * 5)):
        with pytest.raises(ValueError):
            engine.range_fade_replay(*a, **bad)
    with pytest.raises(ValueError):
        engine.range_fade_replay(*a[:9], dv(p["ctx"][:2]), a[10])
    with pytest.raises(ValueError, match="no CPU path"):
        engine.range_fade_replay(*a[:9], torch.from_numpy(p["ctx"]), a[10])
