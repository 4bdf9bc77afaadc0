"""CPU: bq_bb_extreme_replay rejects bad arguments before any launch (no device
is touched: the pointers are fake and never dereferenced, the value table is a
host array) and its default parameters are BBExtremeReversion's."""

import ctypes

import pytest

from binquant_amd import _lib

S, T = 8, 100
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")


def _call(**kw):
    lib = _lib.load()
    a = dict(close=FAKE, ld_px=T, up=FAKE, mid=FAKE, lo=FAKE, ld_bb=T, lens=None, first=None, frm=None, S=S, T=T,
             params=None, status=FAKE, values=_lib.ptr_array([FAKE] * len(_lib.BBX_VALUES)), ld_out=T)
    a.update(kw)
    return lib.bq_bb_extreme_replay(a["close"], a["ld_px"], a["up"], a["mid"], a["lo"], a["ld_bb"], a["lens"],
                                    a["first"], a["frm"], a["S"], a["T"], a["params"], a["status"], a["values"],
                                    a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqBbExtremeParams()
    _lib.load().bq_bb_extreme_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_constants():
    from binquant_amd import engine, signals
    from tests import bbextreme_cases as bc

    p = _lib.BqBbExtremeParams()
    _lib.load().bq_bb_extreme_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqBbExtremeParams._fields_}
    # bb_extreme_reversion.py: LOOKBACK_CANDLES :67, DEFAULT_* :50-55
    assert got == dict(lookback=30, rsi_window=2, oversold_rsi=5.0, overbought_rsi=95.0, max_lower_band_position=0.0,
                       min_upper_band_position=1.0)
    assert got == engine.BB_EXTREME_DEFAULTS == bc.ref.DEFAULTS
    assert list(engine.BB_EXTREME_DEFAULTS) == list(bc.ref.DEFAULTS)
    fx = bc.fixture()   # the class constants as the generator read them from the class
    assert got == dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist()))
    assert ctypes.sizeof(_lib.BqBbExtremeParams) == 2 * 4 + 4 * 8
    assert _lib.BBX_VALUES == signals.BBX_VALUES == bc.ref.VALUES
    assert _lib.BBX_REASONS == bc.ref.REASONS and signals.BBX_REASONS == dict(enumerate(bc.ref.REASONS))
    assert (_lib.BQ_BBX_EMIT, _lib.BQ_BBX_NO_FRAME, _lib.BQ_BBX_NO_EXTREME) == (0, 1, 6)
    assert (signals.BBX_EMIT, signals.BBX_NO_FRAME, signals.BBX_NOT_ENOUGH_DATA, signals.BBX_NULLS, signals.BBX_NO_RSI,
            signals.BBX_INVALID_BAND, signals.BBX_NO_EXTREME) == tuple(range(7))
    assert (signals.BBX_BUY, signals.BBX_SELL) == (bc.ref.BUY, bc.ref.SELL)
    assert signals.BBX_ROUTE_REASONS == bc.ref.ROUTE_REASONS == tuple(fx["reasons"])
    assert _lib.MARKET_REGIMES == bc.ref.MARKET_REGIMES and _lib.MICRO_REGIMES == bc.ref.MICRO_REGIMES
    assert _lib.MICRO_TRANSITIONS == bc.ref.MICRO_TRANSITIONS
    assert signals.BBX_BLOCKING_TRANSITIONS == bc.ref.BLOCKING_TRANSITIONS
    for name in ("market_range_unstable_allowed", "market_range_stable", "symbol_features_unavailable",
                 "symbol_micro_regime_unstable", "symbol_regime_not_shortable", "symbol_regime_trend_down_for_long",
                 "market_regime_none"):
        assert name in signals.BBX_ROUTE_REASONS


@pytest.mark.parametrize("kw", [
    dict(close=None), dict(up=None), dict(mid=None), dict(lo=None), dict(status=None), dict(ld_px=T - 1),
    dict(ld_bb=T - 1), dict(ld_out=T - 1), dict(S=-1), dict(T=-1),
    dict(T=0x80000000, ld_px=0x80000000, ld_bb=0x80000000, ld_out=0x80000000), dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(lookback=0), dict(lookback=-1), dict(lookback=65), dict(rsi_window=0), dict(rsi_window=-3),
    dict(oversold_rsi=NAN), dict(overbought_rsi=INF), dict(max_lower_band_position=-INF),
    dict(min_upper_band_position=NAN),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0) == _lib.BQ_OK
    # rsi_window + 1 > lookback is the method's own "not enough candles" branch, not an error
    assert _call(S=0, values=None, lens=FAKE, first=FAKE, frm=FAKE,
                 params=_params(lookback=64, rsi_window=64)) == _lib.BQ_OK
    assert _call(T=0, params=_params(lookback=1, rsi_window=1_000_000)) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(lookback=65)) == _lib.BQ_EINVAL
