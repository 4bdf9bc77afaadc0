"""GPU: bq_mean_reversion_replay (bq_meanrev.hip) and its Python layers against
what the real method did (tests/golden/meanrev_gates.npz) and, at the
kernel's step edges, against the numpy / pandas restatement that fixture pins
(tests/meanrev_ref.py). Codes, state and repeated messages exact; values bit
for bit with the features given; with the features formed in the pass rsi /
previous_rsi within 1e-9 x 100 absolute (bq_wilder_rsi's bar in
test_signals_gpu.py), volume_ma / atr_ma / trend_score within 1e-9 relative
(SURVEY §8c), score within 1e-9 absolute, stop_loss_pct bit for bit
(meanrev_cases.BARS)."""

import numpy as np
import pytest
import torch

from tests import meanrev_cases as mc
from tests.meanrev_cases import pg, ref

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


def sym_tensors(sym):
    if sym is None:
        return None
    return {"ok": dv(np.asarray(sym["ok"], bool)), "atr_pct": dv(np.asarray(sym["atr_pct"], np.float64)),
            "trend_score": dv(np.asarray(sym["trend_score"], np.float64)),
            "micro_regime": dv(np.asarray(sym["micro_regime"], np.uint8)),
            "micro_transition": dv(np.asarray(sym["micro_transition"], np.uint8))}


def replay(p, *, state=None, pad=0, features=None, columns=ref.VALUES, **kw):
    """signals.mean_reversion_fade_entry on numpy inputs; returns replay()'s
    layout and, with a state, the state after the call."""
    from binquant_amd import signals

    put = (lambda a: pitched(a, pad)) if pad else dv
    for k in ("first_t", "lens", "from_t"):
        if kw.get(k) is not None:
            kw[k] = dv(np.asarray(kw[k], np.int64))
    st = None
    if state is not None:
        st = signals.MeanReversionState(dv(np.asarray(state[0], np.uint8)), dv(np.asarray(state[1], np.int64)))
    ft = {k: put(features[k]) for k in ref.FEATURES} if features is not None else None
    ctx_ok = p.get("ctx_ok")
    out = signals.mean_reversion_fade_entry(
        *(put(p[k]) for k in mc.PANELS), dv(p["open_time"]), dv(p["ctx"]),
        dv(np.asarray(ctx_ok, bool).reshape(-1)) if ctx_ok is not None else None, sym=sym_tensors(p.get("sym")),
        features=ft, state=st, columns=columns, **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    return got, (tuple(x.cpu().numpy() for x in st.tensors()) if st is not None else None)


def fixture_inputs():
    p = dict(mc.panel())
    p["sym"] = pg.sym_of(p)
    return p


def test_fixture_with_features_formed_in_the_pass(cuda):
    fx, p = mc.fixture(), fixture_inputs()
    got, state = replay(p, first_t=p["first_t"], lens=p["lens"], state=(np.zeros(pg.S), np.zeros(pg.S)))
    want = mc.recorded()
    mc.assert_codes_equal(got, want, "kernel, in-pass features")
    mc.assert_values_close(got, want, "kernel, in-pass features")
    mc.assert_state_equal(state, (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")


def test_fixture_with_recorded_features_is_bit_exact(cuda):
    fx, p = mc.fixture(), fixture_inputs()
    ft = mc.recorded_features()
    got, state = replay(p, features=ft, first_t=p["first_t"], lens=p["lens"],
                        state=(np.zeros(pg.S), np.zeros(pg.S)))
    want = mc.recorded()
    mc.assert_codes_equal(got, want, "kernel, features given")
    mc.assert_values_bits(got, want, "kernel, features given")
    mc.assert_state_equal(state, (fx["state_has"][:, -1], fx["state_last"][:, -1]), "final state")
    stateless, _ = replay(p, features=ft, first_t=p["first_t"], lens=p["lens"], pad=7)
    mc.assert_codes_equal(stateless, want, "kernel, no state, pitched rows")
    mc.assert_values_bits(stateless, want, "kernel, no state, pitched rows")


@pytest.mark.parametrize("given", [False, True], ids=["in_pass", "given"])
def test_fixture_repeated_messages(cuda, given):
    """The same candle sent twice: candle_already_emitted the second time
    where it had emitted, its first answer otherwise."""
    fx, p = mc.fixture(), fixture_inputs()
    reps = fx["repeats"]
    by_row = {}
    for i, (s, t) in enumerate(reps):   # one candle per row and call
        by_row.setdefault(int(s), []).append((i, int(t)))
    for k in range(max(len(v) for v in by_row.values())):
        picks = [(s, v[k]) for s, v in sorted(by_row.items()) if len(v) > k]
        rows = [s for s, _ in picks]
        idx = np.array([i for _, (i, _) in picks])
        t = np.array([u for _, (_, u) in picks])
        sub = {key: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (pg.S,) else v) for key, v in p.items()}
        sub["sym"] = {key: v[rows] for key, v in p["sym"].items()}
        ft = {key: v[rows] for key, v in mc.recorded_features().items()} if given else None
        got, after = replay(sub, features=ft, state=(fx["state_has"][rows, t], fx["state_last"][rows, t]),
                            first_t=p["first_t"][rows], lens=t + 1, from_t=t)
        n = np.arange(len(rows))
        assert (got["status"][n, t] == fx["repeat_status"][idx]).all()
        assert (after[1] == fx["repeat_last"][idx]).all()
        assert (np.delete(got["status"][0], t[0]) == ref.NO_FRAME).all()


NAN_CLOSE = [(0, 62), (1, 63), (2, 64), (3, 20), (4, 126), (4, 127), (4, 128)]
NAN_VOLUME = [(0, 63), (1, 64), (2, 82), (3, 5)]


def edge_case(S, T):
    first = np.array([(0, 1, 45, 63, 64)[s % 5] for s in range(S)]).clip(0, max(T - 1, 0))
    p = mc.seeded_panel(S, T, seed=2000 + 7 * T + S, first_t=first, nan_close=NAN_CLOSE, nan_volume=NAN_VOLUME)
    lens = np.array([T if s % 4 else max(T - 3, 1) for s in range(S)])
    return p, first, lens


@pytest.mark.parametrize("T", [1, 15, 20, 21, 63, 64, 65, 83, 84, 129, 257])
@pytest.mark.parametrize("S", [1, 5, 70])
def test_step_edges_vs_restatement(cuda, S, T):
    """Seeded panels dense in setups on a row pitch of T + 7: first_t cycling
    through 0 / 1 / 45 / 63 / 64, lens < T on some rows, a NaN close at lanes
    62 / 63 / 0 of a step (the diff spans the edge), a NaN volume at candles
    63 / 64 / 82, high == low cells, a context per candle with holes, the
    snapshot [S, T]; the features formed in the pass (BARS) and given (bits)."""
    p, first, lens = edge_case(S, T)
    kw = dict(first_t=first, lens=lens, max_trend_score=mc.TREND_CEILING)
    want = mc.ref_replay(p, **kw)
    mc.no_near_ties(dict(p, lens=lens), want, first, max_trend_score=mc.TREND_CEILING)
    got, state = replay(p, pad=7, state=(np.zeros(S), np.zeros(S)), **kw)
    mc.assert_codes_equal(got, want, f"{S}x{T} in-pass features")
    mc.assert_values_close(got, want, f"{S}x{T} in-pass features")
    mc.assert_state_equal(state, want["state"], f"{S}x{T} in-pass features")
    ft = mc.random_features(p, seed=T + S)
    want = mc.ref_replay(p, features_given=ft, **kw)
    got, state = replay(p, pad=7, features=ft, state=(np.zeros(S), np.zeros(S)), **kw)
    mc.assert_codes_equal(got, want, f"{S}x{T} features given")
    mc.assert_values_bits(got, want, f"{S}x{T} features given")
    mc.assert_state_equal(state, want["state"], f"{S}x{T} features given")


def test_optional_inputs(cuda):
    """sym=None, the snapshot [S], one context for every candle, ctx_ok
    absent, status alone."""
    S, T = 5, 130
    kw = dict(max_trend_score=mc.TREND_CEILING)
    p = mc.seeded_panel(S, T, seed=77, per_candle_ctx=False, sym_dims=1, nan_volume=[(0, 70)])
    p["ctx"][:, 0] = (0.1, 0.2, 0.3, -0.2, 0.001)
    q = dict(p, ctx_ok=None)
    want = mc.ref_replay(q, **kw)
    got, _ = replay(q, **kw)
    mc.assert_codes_equal(got, want, "snapshot [S], ctx [5, 1], no ctx_ok")
    mc.assert_values_close(got, want, "snapshot [S], ctx [5, 1], no ctx_ok")
    assert (want["status"] == ref.EMIT).sum() >= 5 and (want["status"] >= ref.SYMBOL_ATR).any()
    q = dict(p, ctx_ok=None, sym=None)
    want = mc.ref_replay(q, **kw)
    got, _ = replay(q, **kw)
    mc.assert_codes_equal(got, want, "sym=None")
    assert not np.isin(want["status"], (ref.SYMBOL_ATR, ref.BREAKOUT_UP, ref.SYMBOL_TREND_UP)).any()
    p["ctx_ok"] = np.array([False])
    want = mc.ref_replay(p, **kw)
    got, _ = replay(p, columns=(), **kw)
    assert set(got) == {"status"}
    mc.assert_codes_equal(got, want, "no context, status alone")
    assert (want["status"] == ref.NO_CONTEXT).any() and not (want["status"] == ref.EMIT).any()


@pytest.mark.parametrize("k", [63, 64, 100])
def test_split_replay_equals_whole(cuda, k):
    """from_t (100: the middle of a step) with the state carried from a first
    call: the two calls together equal one call, bit for bit."""
    S, T = 5, 200
    first = np.array([0, 1, 45, 64, 0])
    p = mc.seeded_panel(S, T, seed=300 + k, first_t=first, nan_close=[(3, 20), (1, k - 1)], nan_volume=[(1, k)])
    kw = dict(first_t=first, max_trend_score=mc.TREND_CEILING)
    for ft in (None, mc.random_features(p, seed=k)):
        whole, end = replay(p, features=ft, state=(np.zeros(S), np.zeros(S)), **kw)
        a, mid = replay(p, features=ft, lens=np.full(S, k), state=(np.zeros(S), np.zeros(S)), **kw)
        b, fin = replay(p, features=ft, from_t=np.full(S, k), state=mid, **kw)
        for name in ("status",) + ref.VALUES:
            joined = np.concatenate([a[name][:, :k], b[name][:, k:]], axis=1)
            same = mc.same_bits(joined, whole[name]) if name in ref.VALUES else joined == whole[name]
            assert same.all(), (name, ft is None, np.argwhere(~same)[:5].tolist())
        assert (b["status"][:, :k] == ref.NO_FRAME).all() and (a["status"][:, k:] == ref.NO_FRAME).all()
        assert (whole["status"] == ref.EMIT).sum() >= 5
        mc.assert_state_equal(fin, end, "split")


def test_entry_is_dropped_by_an_earlier_emit_of_the_same_call(cuda):
    S, T = 5, 130
    p = mc.seeded_panel(S, T, seed=4)
    kw = dict(max_trend_score=mc.TREND_CEILING)
    base = mc.ref_replay(p, **kw)
    row = int(np.argmax((base["status"] == ref.EMIT).sum(axis=1)))
    b = int(np.nonzero(base["status"][row] == ref.EMIT)[0][1])
    has, last = np.zeros(S, bool), np.zeros(S, np.int64)
    has[row], last[row] = True, p["open_time"][row, b]
    for extra in ({}, dict(from_t=np.full(S, b))):
        want = mc.ref_replay(p, state=(has, last), **kw, **extra)
        got, state = replay(p, state=(has, last), **kw, **extra)
        mc.assert_codes_equal(got, want, f"carried entry {extra}")
        mc.assert_state_equal(state, want["state"], f"carried entry {extra}")
    assert want["status"][row, b] == ref.ALREADY_EMITTED


def test_staged_features_pass_through(cuda):
    """The kernel given signals.mean_reversion_features' columns reproduces
    them bit for bit in its value outputs."""
    from binquant_amd import signals

    S, T = 5, 130
    p = mc.seeded_panel(S, T, seed=12)
    cols = [dv(p[k]) for k in mc.PANELS]
    staged = signals.mean_reversion_features(*cols[:6])
    state = signals.MeanReversionState.empty(S, "cuda")
    copy = state.clone()
    out = signals.mean_reversion_fade_entry(*cols, dv(p["open_time"]), dv(p["ctx"]), dv(p["ctx_ok"]),
                                            sym=sym_tensors(p["sym"]), features=staged, state=state,
                                            max_trend_score=mc.TREND_CEILING)
    torch.cuda.synchronize()
    assert set(out) == {"status", *ref.VALUES}
    for k in ref.FEATURES:
        assert mc.same_bits(out[k].cpu().numpy(), staged[k].cpu().numpy()).all(), k
    assert (out["status"] == ref.EMIT).any() and state.has.any()
    assert not copy.has.any() and not copy.last_open_time.any()


def test_engine_value_errors_on_device(cuda):
    """Bad arguments with device tensors: ValueError, nothing launched."""
    from binquant_amd import engine

    p = mc.seeded_panel(3, 40, seed=1)
    a = [dv(p[k]) for k in mc.PANELS] + [dv(p["open_time"]), dv(p["ctx"]), dv(p["ctx_ok"])]
    for bad in (dict(rsi_window=0), dict(nope=1), dict(rsi_short_min=float("nan")), dict(volume_ma_window=65),
                dict(columns=("nope",)), dict(state=(a[9], a[7][:, 0])), dict(features=(a[0],) * 4),
                dict(features=(a[0][:, :5],) * 5), dict(sym=(a[9],) * 5)):
        with pytest.raises(ValueError):
            engine.mean_reversion_replay(*a, **bad)
    with pytest.raises(ValueError):
        engine.mean_reversion_replay(*a[:8], dv(p["ctx"][:4]), a[9])
    with pytest.raises(ValueError):
        engine.mean_reversion_replay(*a[:7], a[7].int(), *a[8:])
