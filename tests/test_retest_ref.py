"""CPU checks of the gradual-gainer retest replay: the numpy restatement
(tests/retest_ref.py) equals what the REAL GradualGainerRetest.signal() did
candle by candle (tests/golden/retest_gates.npz, tests/golden/make_golden_retest.py)
— events, detail bits, levels and the state after every candle, all exact —
the fixture holds what it is for, and the C ABI / engine wrappers reject bad
arguments before a device is touched."""

import ctypes

import numpy as np
import pytest
import torch

from tests import retest_cases as rc
from tests.retest_cases import pg, ref


@pytest.fixture(scope="module")
def restated():
    fx, p = rc.fixture(), rc.panel()
    return ref.retest_replay(*(p[k] for k in rc.COLS), fx["ema"], p["open_time"], fx["leader"], p["risk_ok"],
                             first_t=p["first_t"], lens=p["lens"], from_t=p["first_t"], trace=True,
                             **rc.fixture_params())


def test_restatement_equals_reference(restated):
    fx = rc.fixture()
    rc.assert_replay_equal(restated[:3], (fx["event"], fx["detail"], fx["level"]), "panel")
    assert np.isnan(restated[2][~np.isin(restated[0], (1, 2, 3, 4))]).all()   # a level only where a watch is in force


def test_restatement_state_after_every_candle(restated):
    fx, p = rc.fixture(), rc.panel()
    active, started, level = restated[4]
    replayed = (np.arange(pg.T) >= p["first_t"][:, None]) & (np.arange(pg.T) < p["lens"][:, None])
    want = fx["st_active"]
    assert (active[replayed] == want[replayed]).all()
    on = replayed & want
    assert (started[on] == fx["st_started"][on]).all()
    assert rc.same_bits(level[on], fx["st_level"][on]).all()
    rc.assert_state_equal(restated[3], rc.recorded_state(p["lens"] - 1), "carry-out")


def test_fixture_holds_what_it_is_for():
    """Counted on the recorded outputs alone (make_golden_retest.coverage's
    counts, stored by the generator)."""
    fx = rc.fixture()
    cov = {k: int(v) for k, v in (str(x).split("=") for x in fx["coverage"])}
    assert all(cov[f"code_{k}"] >= 30 for k in range(6)) and cov["expiries"] >= 20, cov
    assert cov["expire_and_reset"] >= 3 and cov["blocked_then_candidate"] >= 5 and cov["gap_expiries"] >= 3, cov
    assert cov["nan_levels"] >= 1 and cov["ties"] == 0, cov
    ev, dt = fx["event"], fx["detail"]
    assert all(int((ev == k).sum()) == cov[f"code_{k}"] for k in range(6))
    assert int(((dt & ref.D_EXPIRED) != 0).sum()) == cov["expiries"]
    assert tuple(str(x) for x in fx["events"]) == ref.RT_EVENTS
    assert tuple(str(x) for x in fx["risk_reasons"]) == ref.RISK_REASONS
    assert rc.fixture_params() == ref.DEFAULTS
    assert np.bincount(fx["risk_reason"], minlength=8).min() >= 8


def test_restatement_split_run_equals_whole():
    """[0, k) then [k, T) with the carried state = the whole run."""
    p = rc.edge_panel(200, seed=7)
    args = [p[k] for k in rc.COLS] + [p["ema"], p["open_time"], p["leader"], p["risk_ok"]]
    whole = ref.retest_replay(*args, **rc.EDGE_PARAMS)
    for k in (64, 130):
        a = ref.retest_replay(*args, lens=np.full(rc.EDGE_S, k), **rc.EDGE_PARAMS)
        b = ref.retest_replay(*args, from_t=np.full(rc.EDGE_S, k), state=a[3], **rc.EDGE_PARAMS)
        rc.assert_replay_equal(a, whole, f"head {k}", slice(0, k))
        rc.assert_replay_equal(b, whole, f"tail {k}", slice(k, None))
        rc.assert_state_equal(b[3], whole[3], f"split {k}")


def test_codes_and_defaults_match_the_library_tables():
    from binquant_amd import _lib, engine, signals

    assert (_lib.BQ_RT_IDLE, _lib.BQ_RT_WATCH_SET, _lib.BQ_RT_WATCHING, _lib.BQ_RT_RISK_BLOCKED, _lib.BQ_RT_CANDIDATE,
            _lib.BQ_RT_SHORT_HISTORY, _lib.BQ_RT_NO_FRAME) == (ref.RT_IDLE, ref.RT_WATCH_SET, ref.RT_WATCHING,
                                                              ref.RT_RISK_BLOCKED, ref.RT_CANDIDATE,
                                                              ref.RT_SHORT_HISTORY, ref.RT_NO_FRAME)
    assert (signals.RT_D_SUPPORT, signals.RT_D_PULLBACK, signals.RT_D_RECLAIM, signals.RT_D_EXPIRED) == (
        ref.D_SUPPORT, ref.D_PULLBACK, ref.D_RECLAIM, ref.D_EXPIRED)
    assert tuple(signals.RT_EVENTS[i] for i in range(6)) == ref.RT_EVENTS and signals.RT_CANDIDATE == ref.RT_CANDIDATE
    assert signals.RISK_REASONS == ref.RISK_REASONS
    assert engine.RETEST_DEFAULTS == ref.DEFAULTS
    d = _lib.BqRetestParams()
    _lib.load().bq_retest_default_params(ctypes.byref(d))
    assert {k: getattr(d, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    assert ctypes.sizeof(_lib.BqRetestParams) == 32


def test_c_abi_rejects_bad_arguments_without_device():
    """BQ_EINVAL before any launch: NULL columns, pitches below T, a partial
    state, breakout_lookback out of range or not below min_history."""
    from binquant_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 256)()
    x = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(params=None, **kw):
        a = dict(open=x, high=x, low=x, close=x, ema=x, ld_in=8, ts=x, ld_ts=8, leader=x, risk=null, ld_b=8, lens=null,
                 first=null, frm=null, S=2, T=8, st_a=null, st_s=null, st_l=null, event=x, detail=null, level=null,
                 ld_out=8)
        a.update(kw)
        p = ctypes.byref(params) if params is not None else None
        return lib.bq_retest_replay(a["open"], a["high"], a["low"], a["close"], a["ema"], a["ld_in"], a["ts"],
                                    a["ld_ts"], a["leader"], a["risk"], a["ld_b"], a["lens"], a["first"], a["frm"],
                                    a["S"], a["T"], p, a["st_a"], a["st_s"], a["st_l"], a["event"], a["detail"],
                                    a["level"], a["ld_out"], null)

    for k in ("open", "high", "low", "close", "ema", "ts", "leader", "event"):
        assert call(**{k: null}) == _lib.BQ_EINVAL, k
    for k in ("ld_in", "ld_ts", "ld_b", "ld_out"):
        assert call(**{k: 7}) == _lib.BQ_EINVAL, k
    assert call(S=-1) == _lib.BQ_EINVAL and call(T=-1) == _lib.BQ_EINVAL
    assert call(st_a=x) == _lib.BQ_EINVAL and call(st_a=x, st_s=x) == _lib.BQ_EINVAL   # all three or none
    for lookback, min_history in ((0, 100), (65, 100), (8, 8), (8, 5), (-1, 100)):
        p = _lib.BqRetestParams(8 * 3_600_000, min_history, lookback, 0.995, 0.96)
        assert call(p) == _lib.BQ_EINVAL, (lookback, min_history)
    assert call(_lib.BqRetestParams(-1, 100, 8, 0.995, 0.96)) == _lib.BQ_EINVAL
    assert call(S=0) == _lib.BQ_OK and call(T=0, ld_in=0, ld_ts=0, ld_b=0, ld_out=0) == _lib.BQ_OK   # nothing to do


def test_engine_rejects_bad_arguments_without_device():
    """ValueError before any device work: the lookback range, dtypes, shapes,
    CPU tensors, unknown parameters."""
    from binquant_amd import engine

    S, T = 2, 120
    f = torch.ones(S, T, dtype=torch.float64)
    ts = torch.arange(T, dtype=torch.int64).expand(S, T).contiguous()
    b = torch.zeros(S, T, dtype=torch.bool)
    good = [f, f, f, f, f, ts, b]
    for kw in (dict(breakout_lookback=0), dict(breakout_lookback=65), dict(breakout_lookback=8, min_history=8),
               dict(breakout_lookback=50, min_history=20), dict(watch_ms=-1), dict(no_such=1)):
        with pytest.raises(ValueError):
            engine.retest_replay(*good, **kw)
    for i, bad in ((0, f.float()), (4, f[:, :-1]), (5, ts.int()), (5, ts[:, :-1]), (6, b.to(torch.uint8)),
                   (6, b[:1])):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            engine.retest_replay(*args)
    with pytest.raises(ValueError, match="CUDA|CPU"):
        engine.retest_replay(*good)   # host tensors: there is no CPU path
    with pytest.raises(ValueError):
        engine.retest_replay(*good, first_t=[0, 0, 0])
    with pytest.raises(ValueError):
        engine.retest_replay(*good, state=(b, ts, f))
