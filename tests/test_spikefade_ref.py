"""CPU checks of the failed-spike-fade replay: the numpy restatement
(tests/spikefade_ref.py) equals what the REAL FailedSpikeFade.signal() did
candle by candle (tests/golden/spikefade_gates.npz, tests/golden/make_golden_spikefade.py)
— events, detail bits, bars, the state after every candle and the allow
helpers' reasons, all exact — the fixture holds what it is for, and the C ABI
/ engine wrappers reject bad arguments before a device is touched."""

import ctypes

import numpy as np
import pytest
import torch

from tests import spikefade_cases as sc
from tests.spikefade_cases import pg, ref


@pytest.fixture(scope="module")
def restated():
    p = sc.panel()
    return sc.replay_ref(sc.fixture_inputs(), first_t=p["first_t"], lens=p["lens"], from_t=p["first_t"], trace=True,
                         **sc.fixture_params())


def test_restatement_equals_reference(restated):
    fx = sc.fixture()
    sc.assert_replay_equal(restated[:3], (fx["event"], fx["detail"], fx["bars"]), "panel")


def test_restatement_state_after_every_candle(restated):
    fx, p = sc.fixture(), sc.panel()
    active, open_time, high, close = restated[4]
    replayed = (np.arange(pg.T) >= p["first_t"][:, None]) & (np.arange(pg.T) < p["lens"][:, None])
    want = fx["st_active"]
    assert (active[replayed] == want[replayed]).all()
    on = replayed & want
    assert (open_time[on] == fx["st_open_time"][on]).all()
    assert sc.same_bits(high[on], fx["st_high"][on]).all() and sc.same_bits(close[on], fx["st_close"][on]).all()
    sc.assert_state_equal(restated[3], sc.recorded_state(p["lens"] - 1), "carry-out")
    # the message text's volumes are the source candle's: gathered at t - bars, they are no state
    rows, cols = np.nonzero(fx["event"] == ref.FS_CANDIDATE)
    src = cols - fx["bars"][rows, cols]
    assert sc.same_bits(p["volume"][rows, src], fx["st_volume"][rows, cols - 1]).all()
    assert sc.same_bits(p["quote_asset_volume"][rows, src], fx["st_quote_asset_volume"][rows, cols - 1]).all()


def test_restatement_repeated_messages():
    """A second message on a source candle (recorded by the generator as
    (row, t) pairs: the reference returned at bars_elapsed <= 0 and left the
    state as it was) is SAME_CANDLE from the recorded state."""
    fx, p = sc.fixture(), sc.panel()
    rep = fx["repeats"]
    assert len(rep) >= 3
    from_t = np.array(p["lens"])
    # rows without a repeat replay nothing; the others their last repeated candle alone
    state = [np.array(x) for x in sc.idle_state(pg.S)]
    for s, t in rep:
        from_t[s] = t
        for dst, src in zip(state, sc.recorded_state(np.array([t]), [s])):
            dst[s] = src[0]
    lens = np.where(from_t < p["lens"], from_t + 1, p["lens"])
    got = sc.replay_ref(sc.fixture_inputs(), first_t=p["first_t"], lens=lens, from_t=from_t, state=state,
                        **sc.fixture_params())
    rows = np.unique(rep[:, 0])
    assert (got[0][rows, from_t[rows]] == ref.FS_SAME_CANDLE).all()
    assert (got[1][rows, from_t[rows]] == 0).all() and (got[2][rows, from_t[rows]] == 0).all()
    sc.assert_state_equal(tuple(x[rows] for x in got[3]), tuple(x[rows] for x in state), "a repeat leaves the state")


def test_fixture_holds_what_it_is_for():
    """The generator's coverage conditions, asserted again on the recorded
    outputs. Every event code of a candle-by-candle replay: a second message
    on one candle is not a column, so SAME_CANDLE is what `repeats` holds."""
    fx, p = sc.fixture(), sc.panel()
    cov = {k: int(v) for k, v in (str(x).split("=") for x in fx["coverage"])}
    ev, dt, br = fx["event"], fx["detail"], fx["bars"]
    assert all(int((ev == k).sum()) == cov[f"code_{k}"] >= 20 for k in range(5)), cov
    cleared, waiting = ev == ref.FS_CLEARED, ev == ref.FS_WAITING
    counts = dict(window_expired=(cleared & ((dt & ref.D_WINDOW_EXPIRED) != 0)).sum(),
                  extension=(cleared & ((dt & ref.D_EXTENSION) != 0)).sum(),
                  waiting_new_high=(waiting & ((dt & ref.D_NEW_HIGH) != 0)).sum(),
                  waiting_market=(waiting & ((dt & ref.D_MARKET) != 0)).sum(),
                  waiting_new_high_only=(waiting & (dt == ref.D_NEW_HIGH)).sum(),
                  idle_market=((ev == ref.FS_IDLE) & ((dt & ref.D_MARKET) != 0)).sum())
    for k, v in counts.items():
        assert int(v) == cov[k] >= 10, (k, int(v), cov)
    assert ((ev == ref.FS_CANDIDATE) & (br == 8)).sum() == cov["candidate_at_8"] >= 3
    assert (cleared & ((dt & ref.D_WINDOW_EXPIRED) != 0) & (br == 9)).sum() == cov["window_at_9"] >= 3
    assert cov["blocked_then_candidate"] >= 5 and cov["nan_window_rows"] >= 2 and cov["ties"] == 0, cov
    assert (p["first_t"] > 0).sum() == cov["late_rows"] >= 3 and len(fx["repeats"]) == cov["repeats"] >= 3
    # blocked, then candidate: counted again here
    n = 0
    for s in range(pg.S):
        blocked = False
        for t in range(pg.T):
            if ev[s, t] == ref.FS_SOURCE_SET:
                blocked = False
            elif ev[s, t] == ref.FS_WAITING and dt[s, t] == ref.D_MARKET:
                blocked = True
            elif ev[s, t] == ref.FS_CANDIDATE:
                n += blocked
    assert n == cov["blocked_then_candidate"]
    assert tuple(str(x) for x in fx["events"]) == ref.FS_EVENTS
    assert tuple(str(x) for x in fx["source_reasons"]) == ref.SPIKE_SOURCE_REASONS
    assert tuple(str(x) for x in fx["market_reasons"]) == ref.SPIKE_MARKET_REASONS
    assert sc.fixture_params() == ref.DEFAULTS
    assert np.bincount(fx["grid_spike_reason"], minlength=4).min() >= 8
    assert np.bincount(np.r_[fx["grid_src_reason"], fx["grid_fail_reason"]], minlength=8).min() >= 8


def test_allow_helpers_restatement_equals_reference():
    """The numpy restatements of source_spike_allows and of the two market
    methods equal the recorded grids and the panel's per-candle recordings."""
    fx, p = sc.fixture(), sc.panel()
    g = pg.source_cases()
    ok, reason = ref.spike_source_allows(*(g[k] for k in sc.SPIKE_FIELDS), float(fx["max_candle_return"]))
    assert (ok == fx["grid_spike_ok"]).all() and (reason == fx["grid_spike_reason"]).all()
    m = pg.market_cases()
    got = ref.spike_fade_market_allows(m["stress"], m["long_score"], m["short_score"], m["context_ok"], m["momentum"],
                                       float(fx["max_market_stress"]), float(fx["min_momentum"]))
    for x, k in zip(got, ("grid_src_ok", "grid_src_reason", "grid_fail_ok", "grid_fail_reason")):
        assert (x == fx[k]).all(), k
    inside = (np.arange(pg.T) >= p["first_t"][:, None]) & (np.arange(pg.T) < p["lens"][:, None])
    ok, reason = ref.spike_source_allows(*(fx[f"spike_{k}"] for k in sc.SPIKE_FIELDS))
    assert (ok == fx["source_ok"])[inside].all() and (reason == fx["source_reason"])[inside].all()
    got = ref.spike_fade_market_allows(p["stress"], p["long_score"], p["short_score"], p["context_ok"], p["momentum"])
    for x, k in zip(got, ("src_market", "src_market_reason", "fail_market", "fail_market_reason")):
        assert (x == fx[k])[inside].all(), k


def test_restatement_split_run_equals_whole():
    """[0, k) then [k, T) with the carried state = the whole run."""
    S = 6
    p = sc.edge_panel(S, 200, seed=7)
    whole = sc.replay_ref(p)
    for k in (64, 130):
        a = sc.replay_ref(p, lens=np.full(S, k))
        b = sc.replay_ref(p, from_t=np.full(S, k), state=a[3])
        sc.assert_replay_equal(a, whole, f"head {k}", slice(0, k))
        sc.assert_replay_equal(b, whole, f"tail {k}", slice(k, None))
        sc.assert_state_equal(b[3], whole[3], f"split {k}")
    assert all((whole[0] == k).sum() >= 5 for k in range(5)), np.bincount(whole[0].ravel(), minlength=6)


def test_codes_and_defaults_match_the_library_tables():
    from binquant_amd import _lib, engine, signals

    assert (_lib.BQ_FS_IDLE, _lib.BQ_FS_SOURCE_SET, _lib.BQ_FS_WAITING, _lib.BQ_FS_CANDIDATE, _lib.BQ_FS_CLEARED,
            _lib.BQ_FS_SAME_CANDLE, _lib.BQ_FS_NO_FRAME) == (ref.FS_IDLE, ref.FS_SOURCE_SET, ref.FS_WAITING,
                                                            ref.FS_CANDIDATE, ref.FS_CLEARED, ref.FS_SAME_CANDLE,
                                                            ref.FS_NO_FRAME)
    assert (signals.FS_D_SOURCE, signals.FS_D_MARKET, signals.FS_D_NEW_HIGH, signals.FS_D_CANDLE_EXPIRED,
            signals.FS_D_WINDOW_EXPIRED, signals.FS_D_EXTENSION) == (
        ref.D_SOURCE, ref.D_MARKET, ref.D_NEW_HIGH, ref.D_CANDLE_EXPIRED, ref.D_WINDOW_EXPIRED, ref.D_EXTENSION)
    assert tuple(signals.FS_EVENTS[i] for i in range(6)) == ref.FS_EVENTS and signals.FS_CANDIDATE == ref.FS_CANDIDATE
    assert signals.SPIKE_SOURCE_REASONS == ref.SPIKE_SOURCE_REASONS
    assert signals.SPIKE_MARKET_REASONS == ref.SPIKE_MARKET_REASONS
    assert engine.SPIKE_FADE_DEFAULTS == ref.DEFAULTS and _lib.SPIKEFADE_MAX_WINDOW == ref.MAX_WINDOW
    d = _lib.BqSpikeFadeParams()
    _lib.load().bq_spike_fade_default_params(ctypes.byref(d))
    assert {k: getattr(d, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    assert ctypes.sizeof(_lib.BqSpikeFadeParams) == 16
    assert "bq_spike_fade_replay" in _lib.SIGNATURES and hasattr(signals, "SpikeFadeState")


def test_c_abi_rejects_bad_arguments_without_device():
    """BQ_EINVAL before any launch: NULL columns, pitches below T (ld_m: 0
    is the shared row), a partial state, window_bars out of range, an
    ext_factor that is not finite."""
    from binquant_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 256)()
    x = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(params=None, **kw):
        a = dict(open=x, high=x, close=x, ld_in=8, ts=x, ld_ts=8, source=x, ld_b=8, src_m=null, fail_m=null, ld_m=0,
                 lens=null, first=null, frm=null, S=2, T=8, st_a=null, st_o=null, st_h=null, st_c=null, event=x,
                 detail=null, bars=null, ld_out=8)
        a.update(kw)
        p = ctypes.byref(params) if params is not None else None
        return lib.bq_spike_fade_replay(a["open"], a["high"], a["close"], a["ld_in"], a["ts"], a["ld_ts"], a["source"],
                                        a["ld_b"], a["src_m"], a["fail_m"], a["ld_m"], a["lens"], a["first"], a["frm"],
                                        a["S"], a["T"], p, a["st_a"], a["st_o"], a["st_h"], a["st_c"], a["event"],
                                        a["detail"], a["bars"], a["ld_out"], null)

    for k in ("open", "high", "close", "ts", "source", "event"):
        assert call(**{k: null}) == _lib.BQ_EINVAL, k
    for k in ("ld_in", "ld_ts", "ld_b", "ld_out", "ld_m"):
        assert call(**{k: 7}) == _lib.BQ_EINVAL, k
    assert call(S=-1) == _lib.BQ_EINVAL and call(T=-1) == _lib.BQ_EINVAL
    for n in (1, 2, 3):   # all four or none
        assert call(**dict(zip(("st_a", "st_o", "st_h", "st_c"), (x,) * n))) == _lib.BQ_EINVAL, n
    for window in (0, -1, 33):
        assert call(_lib.BqSpikeFadeParams(window, 1.06)) == _lib.BQ_EINVAL, window
    for ef in (float("nan"), float("inf"), float("-inf")):
        assert call(_lib.BqSpikeFadeParams(8, ef)) == _lib.BQ_EINVAL, ef
    assert call(S=0) == _lib.BQ_OK   # nothing to do
    assert call(T=0, ld_in=0, ld_ts=0, ld_b=0, ld_out=0) == _lib.BQ_OK
    assert call(S=0, ld_m=8) == _lib.BQ_OK and call(S=0, ld_m=0) == _lib.BQ_OK
    assert call(_lib.BqSpikeFadeParams(32, 1.0), S=0) == _lib.BQ_OK and call(_lib.BqSpikeFadeParams(1, -2.5), S=0) == _lib.BQ_OK


def test_engine_rejects_bad_arguments_without_device():
    """ValueError before any device work: the window range, a non-finite
    factor, dtypes, shapes, CPU tensors, unknown parameters."""
    from binquant_amd import engine

    S, T = 2, 120
    f = torch.ones(S, T, dtype=torch.float64)
    ts = torch.arange(T, dtype=torch.int64).expand(S, T).contiguous()
    b = torch.zeros(S, T, dtype=torch.bool)
    good = [f, f, f, ts, b]
    for kw in (dict(window_bars=0), dict(window_bars=33), dict(ext_factor=float("nan")),
               dict(ext_factor=float("inf")), dict(no_such=1)):
        with pytest.raises(ValueError):
            engine.spike_fade_replay(*good, **kw)
    for i, bad in ((0, f.float()), (1, f[:, :-1]), (3, ts.int()), (3, ts[:, :-1]), (4, b.to(torch.uint8)),
                   (4, b[:1])):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            engine.spike_fade_replay(*args)
    for m in (b.to(torch.uint8), b[:, :-1], b[0, :-1]):
        with pytest.raises(ValueError):
            engine.spike_fade_replay(*good, m)
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, b, b[0])   # one [S, T], one [T]
    with pytest.raises(ValueError, match="CUDA|CPU"):
        engine.spike_fade_replay(*good)   # host tensors: there is no CPU path
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, first_t=[0, 0, 0])
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, state=(b, ts, f, f))
    with pytest.raises(ValueError):
        engine.spike_fade_replay(*good, state=(torch.zeros(S, dtype=torch.uint8), torch.zeros(S, dtype=torch.int64),
                                               torch.zeros(S, dtype=torch.float64)))
