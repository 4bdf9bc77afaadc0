"""CPU: bq_buy_the_dip_replay rejects bad arguments before any launch (no
device is touched: the pointers are fake and never dereferenced, the value
table is a host array) and its default parameters are BuyTheDip's."""

import ctypes

import pytest

from binquant_amd import _lib

S, T = 8, 100
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")


def _call(**kw):
    lib = _lib.load()
    a = dict(close=FAKE, ld_px=T, ct=FAKE, ld_ct=T, ema=None, ld_e=T, mkt=FAKE, regime_T=1, micro=FAKE, ld_m=0,
             lens=None, first=None, frm=None, S=S, T=T, params=None, status=FAKE,
             values=_lib.ptr_array([FAKE] * len(_lib.DIP_VALUES)), ld_out=T)
    a.update(kw)
    return lib.bq_buy_the_dip_replay(
        a["close"], a["ld_px"], a["ct"], a["ld_ct"], a["ema"], a["ld_e"], a["mkt"], a["regime_T"], a["micro"],
        a["ld_m"], a["lens"], a["first"], a["frm"], a["S"], a["T"], a["params"], a["status"], a["values"],
        a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqBuyTheDipParams()
    _lib.load().bq_buy_the_dip_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_constants():
    from binquant_amd import engine, signals
    from tests import dip_cases as dc

    p = _lib.BqBuyTheDipParams()
    _lib.load().bq_buy_the_dip_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqBuyTheDipParams._fields_}
    # buy_the_dip.py: LOOKBACK_CANDLES :36, LOOKBACK_HOURS :35, START_TIME :34, the band :159, the span :67
    assert got == dict(lookback_candles=24, lookback_ms=21_600_000, start_time_ms=1_776_036_060_000,
                       min_change_pct=-5.0, max_change_pct=-2.0, ema_span=20)
    assert got == engine.BUY_THE_DIP_DEFAULTS == dc.ref.DEFAULTS
    assert list(engine.BUY_THE_DIP_DEFAULTS) == list(dc.ref.DEFAULTS)
    fx = dc.fixture()   # the class constants as the generator read them from the class
    assert {k: got[k] for k in fx["class_names"].tolist()} == dict(zip(fx["class_names"].tolist(),
                                                                       fx["class_constants"].tolist()))
    assert ctypes.sizeof(_lib.BqBuyTheDipParams) == 2 * 4 + 2 * 8 + 2 * 8
    assert _lib.DIP_VALUES == ("reference_price", "change_6h", "ema20") == signals.DIP_VALUES == dc.ref.VALUES
    assert _lib.DIP_REASONS == dc.ref.REASONS and signals.DIP_REASONS == dict(enumerate(dc.ref.REASONS))
    assert (_lib.BQ_DIP_EMIT, _lib.BQ_DIP_NO_FRAME, _lib.BQ_DIP_NOT_RECLAIMED) == (0, 1, 7)
    assert (signals.DIP_EMIT, signals.DIP_NO_FRAME, signals.DIP_NOT_READY, signals.DIP_BEFORE_START,
            signals.DIP_NO_REFERENCE, signals.DIP_OUT_OF_BAND, signals.DIP_REGIME_BLOCKED,
            signals.DIP_NOT_RECLAIMED) == tuple(range(8))
    assert signals.DIP_ROUTE_REASONS == dc.ref.ROUTE_REASONS
    assert _lib.MARKET_REGIMES == dc.ref.MARKET_REGIMES and _lib.MICRO_REGIMES == dc.ref.MICRO_REGIMES


@pytest.mark.parametrize("kw", [
    dict(close=None), dict(ct=None), dict(status=None), dict(ld_px=T - 1), dict(ld_ct=T - 1), dict(ld_out=T - 1),
    dict(ema=FAKE, ld_e=T - 1), dict(regime_T=2), dict(regime_T=0), dict(regime_T=T + 1), dict(ld_m=T - 1),
    dict(ld_m=1), dict(S=-1), dict(T=-1),
    dict(T=0x80000000, ld_px=0x80000000, ld_ct=0x80000000, ld_out=0x80000000, regime_T=1),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(lookback_candles=1), dict(lookback_candles=0), dict(lookback_ms=0), dict(lookback_ms=-1), dict(ema_span=0),
    dict(min_change_pct=NAN), dict(max_change_pct=NAN), dict(min_change_pct=-INF), dict(max_change_pct=INF),
    dict(min_change_pct=-2.0), dict(min_change_pct=-1.0),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0) == _lib.BQ_OK
    assert _call(S=0, ema=FAKE, mkt=None, micro=None, values=None, regime_T=7, ld_m=3, lens=FAKE, first=FAKE,
                 frm=FAKE, params=_params(lookback_candles=2, start_time_ms=0)) == _lib.BQ_OK
    assert _call(S=0, mkt=FAKE, regime_T=T, micro=FAKE, ld_m=T) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(ema_span=0)) == _lib.BQ_EINVAL
