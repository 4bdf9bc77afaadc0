"""CPU: bq_price_tracker_replay rejects bad arguments before any launch (no
device is touched: the pointers are fake and never dereferenced, the value
table is a host array) and its default parameters are PriceTracker's."""

import ctypes

import pytest

from binquant_amd import _lib

S, T = 8, 100
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")


def _call(**kw):
    lib = _lib.load()
    a = dict(close=FAKE, high=FAKE, low=FAKE, volume=FAKE, ld_px=T, rsi=FAKE, macd=FAKE, mfi=FAKE, ld_ind=T, ct=FAKE,
             ld_ct=T, trend=None, ld_tr=T, rs=FAKE, ld_rs=0, ctx=FAKE, ld_ctx=1, ctx_ok=None, ctx_T=1, lens=None,
             first=None, frm=None, S=S, T=T, params=None, st_has=None, st_last=None, status=FAKE, detail=FAKE,
             values=_lib.ptr_array([FAKE] * len(_lib.PT_VALUES)), ld_out=T)
    a.update(kw)
    return lib.bq_price_tracker_replay(
        a["close"], a["high"], a["low"], a["volume"], a["ld_px"], a["rsi"], a["macd"], a["mfi"], a["ld_ind"],
        a["ct"], a["ld_ct"], a["trend"], a["ld_tr"], a["rs"], a["ld_rs"], a["ctx"], a["ld_ctx"], a["ctx_ok"],
        a["ctx_T"], a["lens"], a["first"], a["frm"], a["S"], a["T"], a["params"], a["st_has"], a["st_last"],
        a["status"], a["detail"], a["values"], a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqPriceTrackerParams()
    _lib.load().bq_price_tracker_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_attributes():
    from binquant_amd import engine

    p = _lib.BqPriceTrackerParams()
    _lib.load().bq_price_tracker_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqPriceTrackerParams._fields_}
    # price_tracker.py: :177 / :175 / :204-205, :194, :198-203, :59-63, :237-239, :34-35
    assert got == dict(min_history=30, tail_rows=5, span_fast=9, span_slow=21, rsi_max=30.0, macd_max=0.0,
                       mfi_max=20.0, w_rsi=0.35, w_mfi=0.35, w_macd=0.3, macd_scale=100.0, context_weight=0.35,
                       risk_weight=0.35, support_weight=0.2, min_followthrough=-0.2, max_risk=0.6,
                       min_confidence=0.5, cooldown_ms=12 * 300_000)
    assert got == engine.PRICE_TRACKER_DEFAULTS
    assert ctypes.sizeof(_lib.BqPriceTrackerParams) == 4 * 4 + 13 * 8 + 8
    assert len(_lib.PT_VALUES) == 6 and len(_lib.PT_REASONS) == 7 and len(_lib.PT_CTX_ROWS) == 4
    assert (_lib.BQ_PT_EMIT, _lib.BQ_PT_NO_FRAME, _lib.BQ_PT_COOLDOWN) == (0, 1, 6)


@pytest.mark.parametrize("kw", [
    dict(close=None), dict(rsi=None), dict(macd=None), dict(mfi=None), dict(ct=None), dict(rs=None), dict(ctx=None),
    dict(status=None), dict(ld_px=T - 1), dict(ld_ind=T - 1), dict(ld_ct=T - 1), dict(ld_out=T - 1),
    dict(trend=FAKE, ld_tr=T - 1), dict(ld_rs=T - 1), dict(ld_rs=1), dict(ctx_T=2), dict(ctx_T=0),
    dict(ctx_T=T, ld_ctx=T - 1), dict(ld_ctx=0), dict(st_has=FAKE), dict(st_last=FAKE), dict(S=-1), dict(T=-1),
    dict(T=0x80000000, ld_px=0x80000000, ld_ind=0x80000000, ld_ct=0x80000000, ld_out=0x80000000, ctx_T=1),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(min_history=0), dict(tail_rows=0), dict(tail_rows=65), dict(span_fast=0), dict(span_slow=0),
    dict(cooldown_ms=-1), dict(rsi_max=NAN), dict(rsi_max=0.0), dict(mfi_max=0.0), dict(macd_max=INF),
    dict(w_rsi=NAN), dict(w_mfi=INF), dict(w_macd=NAN), dict(macd_scale=INF), dict(context_weight=NAN),
    dict(risk_weight=INF), dict(support_weight=NAN), dict(min_followthrough=NAN), dict(max_risk=INF),
    dict(min_confidence=NAN),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, ctx_T=1) == _lib.BQ_OK
    assert _call(S=0, high=None, low=None, volume=None, detail=None, values=None, ctx_ok=FAKE, st_has=FAKE,
                 st_last=FAKE, trend=FAKE, ld_rs=T, params=_params(cooldown_ms=0)) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(tail_rows=0)) == _lib.BQ_EINVAL
