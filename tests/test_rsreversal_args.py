"""CPU: bq_rs_reversal_replay rejects bad arguments before any launch (no
device is touched: the pointers are fake and never dereferenced, the value
table is a host array), its default parameters are
RelativeStrengthReversalRange's, and engine.rs_reversal_replay raises
ValueError on CPU tensors."""

import ctypes

import pytest
import torch

from binquant_amd import _lib

S, T = 8, 200
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")


def _call(**kw):
    lib = _lib.load()
    a = dict(volume=FAKE, ld_v=T, cok=FAKE, mk=FAKE, ar=FAKE, ctx_T=T, fok=FAKE, rs=FAKE, ld_sym=0, lens=None,
             first=None, frm=None, S=S, T=T, params=None, status=FAKE,
             values=_lib.ptr_array([FAKE] * len(_lib.RSR_VALUES)), ld_out=T)
    a.update(kw)
    return lib.bq_rs_reversal_replay(a["volume"], a["ld_v"], a["cok"], a["mk"], a["ar"], a["ctx_T"], a["fok"], a["rs"],
                                     a["ld_sym"], a["lens"], a["first"], a["frm"], a["S"], a["T"], a["params"],
                                     a["status"], a["values"], a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqRsReversalParams()
    _lib.load().bq_rs_reversal_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_constants():
    from binquant_amd import engine, signals
    from tests import rsreversal_cases as rc

    p = _lib.BqRsReversalParams()
    _lib.load().bq_rs_reversal_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqRsReversalParams._fields_ if k != "reserved"}
    # relative_strength_reversal_range.py:38-41
    assert got == dict(window=96, quantile=0.20, avg_return_max=-0.02, rs_min=0.05)
    assert got == engine.RS_REVERSAL_DEFAULTS == rc.ref.DEFAULTS
    assert list(engine.RS_REVERSAL_DEFAULTS) == list(rc.ref.DEFAULTS)
    fx = rc.fixture()   # the class constants as the generator read them from the class
    assert got == dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist()))
    assert ctypes.sizeof(_lib.BqRsReversalParams) == 2 * 4 + 3 * 8
    assert _lib.RSR_VALUES == signals.RSR_VALUES == rc.ref.VALUES == ("volume_floor",)
    assert _lib.RSR_REASONS == rc.ref.REASONS == tuple(fx["reasons"])
    assert signals.RSR_REASONS == dict(enumerate(rc.ref.REASONS))
    assert (_lib.BQ_RSR_EMIT, _lib.BQ_RSR_NO_FRAME, _lib.BQ_RSR_DEAD_TAPE) == (0, 1, 9)
    assert (signals.RSR_EMIT, signals.RSR_NO_FRAME, signals.RSR_SHORT_FRAME, signals.RSR_NO_CONTEXT,
            signals.RSR_REGIME_NONE, signals.RSR_NOT_RANGE, signals.RSR_MARKET_NOT_WEAK, signals.RSR_NO_FEATURES,
            signals.RSR_RS_INSUFFICIENT, signals.RSR_DEAD_TAPE) == tuple(range(10))
    assert _lib.MARKET_REGIMES == rc.ref.MARKET_REGIMES and _lib.MARKET_REGIMES[rc.ref.RANGE] == "RANGE"
    assert _lib.RSR_MAX_WINDOW == rc.ref.MAX_WINDOW == 192 and signals.RSR_ROUTE == rc.ref.ROUTE


@pytest.mark.parametrize("kw", [
    dict(volume=None), dict(mk=None), dict(ar=None), dict(rs=None), dict(status=None), dict(ld_v=T - 1),
    dict(ld_out=T - 1), dict(ld_sym=T - 1), dict(ld_sym=1), dict(ctx_T=0), dict(ctx_T=2), dict(ctx_T=T + 1),
    dict(S=-1), dict(T=-1), dict(T=0x80000000, ld_v=0x80000000, ld_out=0x80000000, ctx_T=0x80000000),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(window=0), dict(window=-1), dict(window=193), dict(quantile=-0.01), dict(quantile=1.01), dict(quantile=NAN),
    dict(avg_return_max=NAN), dict(avg_return_max=-INF), dict(rs_min=INF), dict(rs_min=NAN),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, ctx_T=1) == _lib.BQ_OK
    assert _call(S=0, values=None, cok=None, fok=None, ctx_T=1, ld_sym=T, lens=FAKE, first=FAKE, frm=FAKE,
                 params=_params(window=192, quantile=1.0)) == _lib.BQ_OK
    assert _call(S=0, params=_params(window=1, quantile=0.0)) == _lib.BQ_OK
    assert _call(S=0, volume=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(window=193)) == _lib.BQ_EINVAL


def test_engine_value_errors_on_cpu_tensors():
    """Nothing is launched: the operands are CPU tensors, or wrong before that matters."""
    from binquant_amd import engine

    s, t = 3, 120
    v = torch.rand(s, t, dtype=torch.float64)
    ok, mk, ar = torch.ones(t, dtype=torch.bool), torch.full((t,), 2, dtype=torch.int8), torch.full((t,), -0.05).double()
    fok, rs = torch.ones(s, dtype=torch.bool), torch.full((s,), 0.1, dtype=torch.float64)
    good = (v, ok, mk, ar, fok, rs)
    with pytest.raises(ValueError, match="CUDA"):
        engine.rs_reversal_replay(*good)
    for bad in (dict(window=0), dict(window=193), dict(quantile=1.5), dict(quantile=-0.1), dict(nope=1),
                dict(rs_min=NAN), dict(avg_return_max=INF), dict(columns=("nope",)), dict(first_t=[0, 1]),
                dict(lens=torch.ones(s))):
        with pytest.raises(ValueError):
            engine.rs_reversal_replay(*good, **bad)
    for args in ((v.float(), ok, mk, ar, fok, rs), (v[0], ok, mk, ar, fok, rs), (v, ok[:5], mk, ar, fok, rs),
                 (v, ok.double(), mk, ar, fok, rs), (v, ok, mk.long(), ar, fok, rs), (v, ok, None, ar, fok, rs),
                 (v, ok, mk[:7], ar, fok, rs), (v, ok, mk, ar.float(), fok, rs), (v, ok, mk, ar[:1], fok, rs),
                 (v, ok, mk, ar, fok[:2], rs), (v, ok, mk, ar, fok.double(), rs), (v, ok, mk, ar, fok, rs.float()),
                 (v, ok, mk, ar, fok, rs[:2]), (v, ok, mk, ar, fok, rs.reshape(s, 1).expand(s, t)),
                 (v, ok, mk, ar, None, None)):
        with pytest.raises(ValueError):
            engine.rs_reversal_replay(*args)
