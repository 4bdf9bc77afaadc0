"""CPU: bq_range_fade_replay rejects bad arguments before any launch (no device
is touched: the pointers are fake and never dereferenced, the value and
feature tables are host arrays), its default parameters are
RangeBbRsiMeanReversion's, and engine.range_fade_replay raises ValueError
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
    a = dict(open=FAKE, high=FAKE, low=FAKE, close=FAKE, volume=FAKE, ld_px=T, rsi=FAKE, ld_rsi=T, bbu=FAKE, bbm=FAKE,
             bbl=FAKE, ld_bb=T, features=None, ld_ft=T, ctx=FAKE, ld_ctx=1, ctx_ok=None, ctx_T=1, sym_ok=None,
             sym_regime=None, sym_transition=None, sym_atr=None, sym_bbw=None, ld_sym=0, lens=None, first=None,
             frm=None, S=S, T=T, params=None, status=FAKE, values=_lib.ptr_array([FAKE] * len(_lib.RF_VALUES)),
             ld_out=T)
    a.update(kw)
    return lib.bq_range_fade_replay(
        a["open"], a["high"], a["low"], a["close"], a["volume"], a["ld_px"], a["rsi"], a["ld_rsi"], a["bbu"],
        a["bbm"], a["bbl"], a["ld_bb"], a["features"], a["ld_ft"], a["ctx"], a["ld_ctx"], a["ctx_ok"], a["ctx_T"],
        a["sym_ok"], a["sym_regime"], a["sym_transition"], a["sym_atr"], a["sym_bbw"], a["ld_sym"], a["lens"],
        a["first"], a["frm"], a["S"], a["T"], a["params"], a["status"], a["values"], a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqRangeFadeParams()
    _lib.load().bq_range_fade_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


FEATS = _lib.ptr_array([FAKE] * _lib.RF_NFEATURES)
SYM = dict(sym_ok=FAKE, sym_regime=FAKE, sym_transition=FAKE, sym_atr=FAKE, sym_bbw=FAKE)


def test_default_params_are_the_class_attributes():
    from binquant_amd import engine

    p = _lib.BqRangeFadeParams()
    _lib.load().bq_range_fade_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqRangeFadeParams._fields_ if k != "reserved"}
    # range_bb_rsi_mean_reversion.py:37-51
    assert got == dict(min_candles=40, adx_window=14, zscore_window=20, adx_max=32.0, long_rsi_max=35.0,
                       short_rsi_min=65.0, long_zscore_max=-2.0, short_zscore_min=2.0, band_touch_tolerance=0.002,
                       max_market_stress=0.35, max_symbol_atr_pct=0.04, max_symbol_bb_width=0.08,
                       min_rejection_wick_frac=0.30, long_close_position_min=0.55, short_close_position_max=0.45)
    assert got == engine.RANGE_FADE_DEFAULTS and p.reserved == 0
    assert ctypes.sizeof(_lib.BqRangeFadeParams) == 4 * 4 + 12 * 8
    assert len(_lib.RF_VALUES) == 4 and len(_lib.RF_REASONS) == 15 and len(_lib.RF_CTX_ROWS) == 3
    assert _lib.RF_REASONS.index("emit") == 0 and _lib.RF_REASONS.index("no_bb_rsi_rejection_setup") == 14
    assert _lib.RF_REASONS.index("adx_too_high") == 13 and _lib.RF_REASONS.index("not_enough_data") == 2
    assert _lib.MARKET_REGIMES.index("RANGE") == 2 and _lib.MICRO_REGIMES.index("RANGE") == 2   # BQ_RF_REGIME_RANGE
    assert [_lib.MICRO_TRANSITIONS.index(k) for k in ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN")] == [0, 1, 2]
    assert _lib.RF_VALUES[:_lib.RF_NFEATURES] == ("adx", "zscore")


@pytest.mark.parametrize("kw", [
    dict(open=None), dict(high=None), dict(low=None), dict(close=None), dict(volume=None), dict(rsi=None),
    dict(bbu=None), dict(bbm=None), dict(bbl=None), dict(ctx=None), dict(status=None), dict(ld_px=T - 1),
    dict(ld_rsi=T - 1), dict(ld_bb=T - 1), dict(ld_out=T - 1), dict(features=FEATS, ld_ft=T - 1),
    dict(features=_lib.ptr_array([FAKE, 0])), dict(ld_sym=T - 1), dict(ld_sym=1), dict(ctx_T=2), dict(ctx_T=0),
    dict(ctx_T=T, ld_ctx=T - 1), dict(ld_ctx=0), dict(sym_ok=FAKE), dict(SYM, sym_regime=None),
    dict(SYM, sym_transition=None), dict(SYM, sym_atr=None), dict(SYM, sym_bbw=None), dict(S=-1), dict(T=-1),
    dict(T=0x80000000, ld_px=0x80000000, ld_rsi=0x80000000, ld_bb=0x80000000, ld_out=0x80000000, ctx_T=1),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(min_candles=0), dict(adx_window=0), dict(adx_window=33), dict(zscore_window=0), dict(zscore_window=65),
    dict(adx_max=NAN), dict(adx_max=0.0), dict(long_rsi_max=0.0), dict(long_rsi_max=INF), dict(short_rsi_min=NAN),
    dict(long_zscore_max=NAN), dict(short_zscore_min=INF), dict(band_touch_tolerance=NAN),
    dict(max_market_stress=INF), dict(max_symbol_atr_pct=NAN), dict(max_symbol_bb_width=INF),
    dict(min_rejection_wick_frac=NAN), dict(long_close_position_min=NAN), dict(short_close_position_max=INF),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, ctx_T=1) == _lib.BQ_OK
    assert _call(S=0, features=FEATS, values=None, ctx_ok=FAKE, ld_sym=T, **SYM,
                 params=_params(adx_window=32, zscore_window=64, min_candles=1)) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(adx_window=0)) == _lib.BQ_EINVAL


def _host_args(S=3, T=40):
    z = torch.zeros((S, T), dtype=torch.float64)
    return [z] * 9 + [torch.zeros((3, 1), dtype=torch.float64)]


def _sym(n=3, **repl):
    d = dict(ok=torch.zeros(n, dtype=torch.uint8), micro_regime=torch.zeros(n, dtype=torch.uint8),
             micro_transition=torch.zeros(n, dtype=torch.uint8), atr_pct=torch.zeros(n, dtype=torch.float64),
             bb_width=torch.zeros(n, dtype=torch.float64))
    d.update(repl)
    return tuple(d.values())


@pytest.mark.parametrize("bad", [
    dict(nope=1), dict(min_candles=0), dict(adx_window=0), dict(adx_window=33), dict(zscore_window=0),
    dict(zscore_window=65), dict(adx_max=NAN), dict(adx_max=0.0), dict(long_rsi_max=0.0), dict(short_rsi_min=INF),
    dict(columns=("nope",)), dict(columns=("adx", "rsi")),
    dict(features=(torch.zeros((3, 40), dtype=torch.float64),)),
    dict(features=(torch.zeros((3, 39), dtype=torch.float64),) * 2),
    dict(features=(torch.zeros((3, 40), dtype=torch.float32),) * 2),
    dict(sym=_sym()[:4]), dict(sym=_sym(atr_pct=torch.zeros(3, dtype=torch.float32))),
    dict(sym=_sym(micro_regime=torch.zeros(3, dtype=torch.int64))), dict(sym=_sym(4)),
    dict(sym=_sym(bb_width=torch.zeros((3, 40), dtype=torch.float64))),     # mixed [S] and [S, T]
    dict(sym=_sym(ok=torch.zeros((3, 40), dtype=torch.uint8))),
    dict(lens=[1, 2]), dict(first_t=torch.zeros(3)), dict(from_t=[0] * 4),
    dict(ctx_ok=torch.zeros(2, dtype=torch.bool)), dict(ctx_ok=torch.zeros(1, dtype=torch.float64)),
], ids=lambda kw: ",".join(kw))
def test_engine_value_errors_before_any_device_call(bad):
    """Host tensors throughout: a device call would fail differently (there is
    no CPU path), so ValueError here means the check came first."""
    from binquant_amd import engine

    a = _host_args()
    bad = dict(bad)
    ctx_ok = bad.pop("ctx_ok", None)
    with pytest.raises(ValueError):
        engine.range_fade_replay(*a, ctx_ok, **bad)


def test_engine_rejects_shapes_and_dtypes_before_any_device_call():
    from binquant_amd import engine

    a = _host_args()
    for i, repl in ((0, a[0].float()), (4, a[4][:, :39]), (5, a[5][0]), (5, a[5].float()), (6, a[6][:, :5]),
                    (7, a[7].int()), (8, a[8][:2]), (9, torch.zeros((2, 1), dtype=torch.float64)),
                    (9, torch.zeros((5, 1), dtype=torch.float64)), (9, torch.zeros((3, 2), dtype=torch.float64)),
                    (9, torch.zeros((3, 1), dtype=torch.float32)), (9, torch.zeros(3, dtype=torch.float64)),
                    (3, a[3][0])):
        b = list(a)
        b[i] = repl
        with pytest.raises(ValueError):
            engine.range_fade_replay(*b)
    with pytest.raises(ValueError, match="no CPU path"):   # well-formed host tensors, a non-CUDA ctx: no CPU path
        engine.range_fade_replay(*a)
    with pytest.raises(ValueError, match="no CPU path"):
        engine.range_fade_replay(*a, sym=_sym())


def test_signals_entry_checks_its_dictionaries():
    from binquant_amd import signals

    a = _host_args()
    with pytest.raises(ValueError, match="sym: missing"):
        signals.range_fade_entry(*a, sym={"ok": a[0]})
    with pytest.raises(ValueError, match="features: missing"):
        signals.range_fade_entry(*a, features={"adx": a[0]})
    with pytest.raises(ValueError, match="unknown parameters"):
        signals.range_fade_entry(*a, adx_windw=14)
    assert signals.RF_REASONS[13] == "adx_too_high" and signals.RF_VALUES == _lib.RF_VALUES
    assert signals.RF_SYM_KEYS == ("ok", "micro_regime", "micro_transition", "atr_pct", "bb_width")
