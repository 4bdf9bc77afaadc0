"""CPU: bq_mean_reversion_replay rejects bad arguments before any launch (no
device is touched: the pointers are fake and never dereferenced, the value and
feature tables are host arrays), its default parameters are
MeanReversionFade's, and engine.mean_reversion_replay raises ValueError
before any device call."""

import ctypes

import pytest
import torch

from binquant_amd import _lib

S, T = 8, 100
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")


def _call(**kw):
    lib = _lib.load()
    a = dict(open=FAKE, high=FAKE, low=FAKE, close=FAKE, volume=FAKE, ld_px=T, atr=FAKE, ld_atr=T, bb=FAKE, ld_bb=T,
             ot=FAKE, ld_ot=T, features=None, ld_ft=T, ctx=FAKE, ld_ctx=1, ctx_ok=None, ctx_T=1, sym_ok=None,
             sym_atr=None, sym_trend=None, sym_regime=None, sym_transition=None, ld_sym=0, lens=None, first=None,
             frm=None, S=S, T=T, params=None, st_has=None, st_last=None, status=FAKE,
             values=_lib.ptr_array([FAKE] * len(_lib.MR_VALUES)), ld_out=T)
    a.update(kw)
    return lib.bq_mean_reversion_replay(
        a["open"], a["high"], a["low"], a["close"], a["volume"], a["ld_px"], a["atr"], a["ld_atr"], a["bb"],
        a["ld_bb"], a["ot"], a["ld_ot"], a["features"], a["ld_ft"], a["ctx"], a["ld_ctx"], a["ctx_ok"], a["ctx_T"],
        a["sym_ok"], a["sym_atr"], a["sym_trend"], a["sym_regime"], a["sym_transition"], a["ld_sym"], a["lens"],
        a["first"], a["frm"], a["S"], a["T"], a["params"], a["st_has"], a["st_last"], a["status"], a["values"],
        a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqMeanReversionParams()
    _lib.load().bq_mean_reversion_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


FEATS = _lib.ptr_array([FAKE] * _lib.MR_NFEATURES)
SYM = dict(sym_ok=FAKE, sym_atr=FAKE, sym_trend=FAKE, sym_regime=FAKE, sym_transition=FAKE)


def test_default_params_are_the_class_attributes():
    from binquant_amd import engine

    p = _lib.BqMeanReversionParams()
    _lib.load().bq_mean_reversion_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqMeanReversionParams._fields_ if k != "reserved"}
    # mean_reversion_fade.py:52-73
    assert got == dict(rsi_window=14, volume_ma_window=20, atr_ma_window=20, ema_fast=20, ema_slow=50,
                       rsi_short_min=76.0, volume_ratio_min=0.8, atr_spike_max=2.2, atr_stop_mult=2.0,
                       max_entry_stop_loss_pct=1.5, max_trend_score=0.005, max_market_stress=0.25, max_gap=0.02,
                       max_symbol_atr_pct=0.03, min_wick_ratio=0.0)
    assert got == engine.MEAN_REVERSION_DEFAULTS and p.reserved == 0
    assert ctypes.sizeof(_lib.BqMeanReversionParams) == 6 * 4 + 10 * 8
    assert len(_lib.MR_VALUES) == 7 and len(_lib.MR_REASONS) == 17 and len(_lib.MR_CTX_ROWS) == 5
    assert _lib.MR_REASONS.index("emit") == 0 and _lib.MR_REASONS.index("entry_stop_loss_too_wide") == 16
    assert _lib.MICRO_REGIMES.index("TREND_UP") == 0 and _lib.MICRO_TRANSITIONS.index("BREAKOUT_UP") == 1   # BQ_MR_*
    assert _lib.MR_VALUES[:_lib.MR_NFEATURES] == ("rsi", "previous_rsi", "volume_ma", "atr_ma", "trend_score")


@pytest.mark.parametrize("kw", [
    dict(open=None), dict(high=None), dict(low=None), dict(close=None), dict(volume=None), dict(atr=None),
    dict(bb=None), dict(ot=None), dict(ctx=None), dict(status=None), dict(ld_px=T - 1), dict(ld_atr=T - 1),
    dict(ld_bb=T - 1), dict(ld_ot=T - 1), dict(ld_out=T - 1), dict(features=FEATS, ld_ft=T - 1),
    dict(features=_lib.ptr_array([FAKE, FAKE, 0, FAKE, FAKE])), dict(ld_sym=T - 1), dict(ld_sym=1), dict(ctx_T=2),
    dict(ctx_T=0), dict(ctx_T=T, ld_ctx=T - 1), dict(ld_ctx=0), dict(st_has=FAKE), dict(st_last=FAKE),
    dict(sym_ok=FAKE), dict(SYM, sym_regime=None), dict(SYM, sym_atr=None), dict(S=-1), dict(T=-1),
    dict(T=0x80000000, ld_px=0x80000000, ld_atr=0x80000000, ld_bb=0x80000000, ld_ot=0x80000000, ld_out=0x80000000,
         ctx_T=1),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(rsi_window=0), dict(volume_ma_window=0), dict(volume_ma_window=65), dict(atr_ma_window=0),
    dict(atr_ma_window=65), dict(ema_fast=0), dict(ema_slow=0), dict(rsi_short_min=NAN), dict(rsi_short_min=100.0),
    dict(volume_ratio_min=INF), dict(atr_spike_max=NAN), dict(atr_stop_mult=INF), dict(max_entry_stop_loss_pct=NAN),
    dict(max_trend_score=NAN), dict(max_market_stress=INF), dict(max_gap=NAN), dict(max_symbol_atr_pct=INF),
    dict(min_wick_ratio=NAN),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, ctx_T=1) == _lib.BQ_OK
    assert _call(S=0, features=FEATS, values=None, ctx_ok=FAKE, st_has=FAKE, st_last=FAKE, ld_sym=T, **SYM,
                 params=_params(volume_ma_window=64, atr_ma_window=1)) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(rsi_window=0)) == _lib.BQ_EINVAL


def _host_args(S=3, T=40):
    z = torch.zeros((S, T), dtype=torch.float64)
    return [z] * 7 + [torch.zeros((S, T), dtype=torch.int64), torch.zeros((5, 1), dtype=torch.float64)]


@pytest.mark.parametrize("bad", [
    dict(nope=1), dict(rsi_window=0), dict(volume_ma_window=65), dict(atr_ma_window=0), dict(ema_fast=0),
    dict(ema_slow=0), dict(rsi_short_min=NAN), dict(rsi_short_min=100.0), dict(max_trend_score=INF),
    dict(columns=("nope",)), dict(features=(torch.zeros((3, 40), dtype=torch.float64),) * 4),
    dict(features=(torch.zeros((3, 39), dtype=torch.float64),) * 5),
    dict(features=(torch.zeros((3, 40), dtype=torch.float32),) * 5),
    dict(sym=(torch.zeros(3, dtype=torch.uint8),) * 4),
    dict(sym=(torch.zeros(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.float32),
              torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.uint8),
              torch.zeros(3, dtype=torch.uint8))),
    dict(sym=(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.float64),
              torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.uint8),
              torch.zeros(4, dtype=torch.uint8))),
    dict(state=(torch.zeros(3, dtype=torch.uint8),)),
    dict(state=(torch.zeros(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32))),
    dict(lens=[1, 2]), dict(first_t=torch.zeros(3)), dict(from_t=[0] * 4),
    dict(ctx_ok=torch.zeros(2, dtype=torch.bool)), dict(ctx_ok=torch.zeros(1, dtype=torch.float64)),
], ids=lambda kw: ",".join(kw))
def test_engine_value_errors_before_any_device_call(bad):
    """Host tensors throughout: a device call would fail differently (there is
    no CPU path), so ValueError here means the check came first."""
    from binquant_amd import engine

    a = _host_args()
    ctx_ok = bad.pop("ctx_ok", None)
    with pytest.raises(ValueError):
        engine.mean_reversion_replay(*a, ctx_ok, **bad)


def test_engine_rejects_shapes_and_dtypes_before_any_device_call():
    from binquant_amd import engine

    a = _host_args()
    for i, repl in ((0, a[0].float()), (5, a[5][:, :39]), (6, a[6][0]), (7, a[7].int()), (7, a[7][:, :5]),
                    (8, torch.zeros((4, 1), dtype=torch.float64)), (8, torch.zeros((5, 2), dtype=torch.float64)),
                    (8, torch.zeros((5, 1), dtype=torch.float32)), (3, a[3][0])):
        b = list(a)
        b[i] = repl
        with pytest.raises(ValueError):
            engine.mean_reversion_replay(*b)
    with pytest.raises(ValueError, match="no CPU path"):   # well-formed host tensors: still no CPU path
        engine.mean_reversion_replay(*a)


def test_signals_entry_checks_its_dictionaries():
    from binquant_amd import signals

    a = _host_args()
    with pytest.raises(ValueError, match="sym: missing"):
        signals.mean_reversion_fade_entry(*a, sym={"ok": a[0]})
    with pytest.raises(ValueError, match="features: missing"):
        signals.mean_reversion_fade_entry(*a, features={"rsi": a[0]})
    assert signals.MR_REASONS[15] == "candle_already_emitted" and signals.MR_VALUES == _lib.MR_VALUES
