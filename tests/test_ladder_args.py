"""CPU: bq_grid_ladder_replay rejects bad arguments before any launch (no
device is touched: the pointers are fake and never dereferenced, the value
table is a host array), its default parameters are LadderDeployer's class
constants, and signals.grid_ladder_entry raises ValueError on mismatched
shapes or dtypes and on CPU tensors."""

import ctypes

import pytest
import torch

from binquant_amd import _lib

S, T = 8, 200
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")
SYM = ("sok", "sreg", "strans", "e20", "e50", "srs", "satr")


def _call(**kw):
    lib = _lib.load()
    a = dict(close=FAKE, ld_c=T, bbu=FAKE, bbm=FAKE, bbl=FAKE, ld_bb=T, high=FAKE + 8, mid=FAKE + 8, low=FAKE + 8,
             ld_bands=T, pok=FAKE, cok=FAKE, mk=FAKE, score=FAKE, ctx_T=T, ld_sym=0, lens=None, first=None, frm=None,
             S=S, T=T, params=None, status=FAKE, values=_lib.ptr_array([FAKE] * len(_lib.GL_VALUES)), ld_out=T,
             **{k: FAKE for k in SYM})
    a.update(kw)
    return lib.bq_grid_ladder_replay(
        a["close"], a["ld_c"], a["bbu"], a["bbm"], a["bbl"], a["ld_bb"], a["high"], a["mid"], a["low"], a["ld_bands"],
        a["pok"], a["cok"], a["mk"], a["score"], a["ctx_T"], *(a[k] for k in SYM), a["ld_sym"], a["lens"], a["first"],
        a["frm"], a["S"], a["T"], a["params"], a["status"], a["values"], a["ld_out"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqGridLadderParams()
    _lib.load().bq_grid_ladder_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_constants():
    from binquant_amd import engine, signals
    from tests import ladder_cases as lc

    p = _lib.BqGridLadderParams()
    _lib.load().bq_grid_ladder_default_params(ctypes.byref(p))
    got = {k: getattr(p, k) for k, _ in _lib.BqGridLadderParams._fields_ if k != "reserved"}
    # ladder_deployer.py:16-28
    assert got == dict(n=8, max_change_pct=20.0, min_width_pct=1.5, max_width_pct=8.0, min_buffer_pct=0.5,
                       max_buffer_pct=4.0, atr_multiplier=1.5, min_long_score=0.2)
    assert got == engine.GRID_LADDER_DEFAULTS == lc.ref.DEFAULTS
    assert list(engine.GRID_LADDER_DEFAULTS) == list(lc.ref.DEFAULTS)
    fx = lc.fixture()   # the class constants as the generator read them from the class
    assert got == dict(zip(fx["default_names"].tolist(), fx["defaults"].tolist()))
    assert ctypes.sizeof(_lib.BqGridLadderParams) == 2 * 4 + 7 * 8
    assert _lib.GL_VALUES == signals.GL_VALUES == lc.ref.VALUES and len(_lib.GL_VALUES) == 5
    assert _lib.GL_REASONS == lc.ref.REASONS == tuple(fx["reasons"])
    assert signals.GL_REASONS == dict(enumerate(lc.ref.REASONS))
    assert (signals.GL_EMIT, signals.GL_NO_FRAME, signals.GL_POLICY, signals.GL_NO_CONTEXT, signals.GL_NOT_RANGE,
            signals.GL_MICRO_REGIME, signals.GL_SYMBOL_TRANSITION, signals.GL_BELOW_EMAS, signals.GL_RS_NOT_POSITIVE,
            signals.GL_LONG_SCORE_LOW, signals.GL_BB_EXPANDING, signals.GL_PRICE_OUTSIDE,
            signals.GL_RANGE_WIDTH) == tuple(range(13))
    assert (_lib.BQ_GL_EMIT, _lib.BQ_GL_NO_FRAME, _lib.BQ_GL_RANGE_WIDTH) == (0, 1, 12)
    assert signals.GL_SYM_KEYS == lc.ref.SYM_KEYS and signals.GL_CTX_ROWS == ("market_regime", "long_regime_score")
    assert signals.GL_BLOCKING_TRANSITIONS == lc.ref.BLOCKING_TRANSITIONS
    assert _lib.MARKET_REGIMES == lc.ref.MARKET_REGIMES and _lib.MICRO_REGIMES == lc.ref.MICRO_REGIMES
    assert _lib.MICRO_TRANSITIONS == lc.ref.MICRO_TRANSITIONS and _lib.MR_NONE == lc.ref.NONE
    assert _lib.MARKET_REGIMES[lc.ref.RANGE] == _lib.MICRO_REGIMES[lc.ref.RANGE] == "RANGE"
    assert _lib.GRID_LADDER_TILE == engine.GRID_LADDER_TILE == lc.ref.TILE
    assert _lib.BB_STABLE_MAX_N == lc.ref.MAX_N


@pytest.mark.parametrize("kw", [
    dict(close=None), dict(bbu=None), dict(bbm=None), dict(bbl=None), dict(mk=None), dict(score=None),
    dict(status=None), dict(high=None), dict(mid=None), dict(low=None), dict(high=None, mid=None),
    dict(ld_c=T - 1), dict(ld_bb=T - 1), dict(ld_bands=T - 1), dict(ld_out=T - 1), dict(ld_sym=T - 1), dict(ld_sym=1),
    dict(ctx_T=0), dict(ctx_T=2), dict(ctx_T=T + 1), dict(S=-1), dict(T=-1), dict(sreg=None), dict(strans=None),
    dict(e20=None), dict(e50=None), dict(srs=None), dict(satr=None),
    dict(T=0x80000000, ld_c=0x80000000, ld_bb=0x80000000, ld_bands=0x80000000, ld_out=0x80000000, ctx_T=0x80000000),
    dict(S=0x200000000),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=-1), dict(n=65), dict(max_change_pct=NAN), dict(min_width_pct=INF), dict(max_width_pct=NAN),
    dict(min_buffer_pct=-INF), dict(max_buffer_pct=NAN), dict(atr_multiplier=INF), dict(min_long_score=NAN),
], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, ctx_T=1) == _lib.BQ_OK
    # every optional pointer absent: the bands are the frame's, no policy, a context everywhere, no symbol features
    assert _call(S=0, values=None, high=None, mid=None, low=None, ld_bands=0, pok=None, cok=None, ctx_T=1, ld_sym=T,
                 lens=FAKE, first=FAKE, frm=FAKE, params=_params(n=64), **{k: None for k in SYM}) == _lib.BQ_OK
    assert _call(S=0, params=_params(n=1)) == _lib.BQ_OK
    assert _call(S=0, close=None) == _lib.BQ_EINVAL   # the checks come first
    assert _call(S=0, params=_params(n=65)) == _lib.BQ_EINVAL


def _good(s=3, t=120):
    c = torch.rand(s, t, dtype=torch.float64) + 10.0
    ctx = torch.zeros(2, t, dtype=torch.float64)
    sym = dict(ok=torch.ones(s, dtype=torch.bool), micro_regime=torch.full((s,), 2, dtype=torch.uint8),
               micro_transition=torch.full((s,), 255, dtype=torch.uint8), above_ema20=torch.ones(s, dtype=torch.bool),
               above_ema50=torch.ones(s, dtype=torch.bool), rs_vs_btc=torch.full((s,), 0.1, dtype=torch.float64),
               atr_pct=torch.full((s,), 0.01, dtype=torch.float64))
    return [c, c + 1.0, c.clone(), c - 1.0, ctx], dict(ctx_ok=torch.ones(t, dtype=torch.bool),
                                                       policy_ok=torch.ones(t, dtype=torch.bool), sym=sym)


def test_entry_value_errors_on_cpu_tensors():
    """Nothing is launched: the operands are CPU tensors, or wrong before that matters."""
    from binquant_amd import signals

    s, t = 3, 120
    args, kw = _good(s, t)
    with pytest.raises(ValueError, match="CUDA"):
        signals.grid_ladder_entry(*args, **kw)
    for bad in (dict(n=0), dict(n=65), dict(nope=1), dict(max_change_pct=NAN), dict(min_long_score=INF),
                dict(columns=("nope",)), dict(first_t=[0, 1]), dict(lens=torch.ones(s)), dict(from_t=[0] * (s + 1)),
                dict(bands=(args[1], args[2])), dict(bands=(args[1], args[2], args[3][:, :5])),
                dict(bands=(args[1].float(), args[2], args[3])), dict(ctx_ok=torch.ones(t - 1, dtype=torch.bool)),
                dict(ctx_ok=torch.ones(t)), dict(policy_ok=torch.ones(1, dtype=torch.bool)),
                dict(policy_ok=torch.ones(t, dtype=torch.int8)),
                dict(sym={k: v for k, v in kw["sym"].items() if k != "atr_pct"}),
                dict(sym=dict(kw["sym"], ok=torch.ones(s + 1, dtype=torch.bool))),
                dict(sym=dict(kw["sym"], micro_regime=torch.full((s,), 2, dtype=torch.int8))),
                dict(sym=dict(kw["sym"], rs_vs_btc=torch.full((s,), 0.1))),
                dict(sym=dict(kw["sym"], atr_pct=torch.full((s, t), 0.01, dtype=torch.float64)))):
        with pytest.raises(ValueError):
            signals.grid_ladder_entry(*args, **{**kw, **bad})
    c, up, md, lw, ctx = args
    for wrong in ((c.float(), up, md, lw, ctx), (c[0], up, md, lw, ctx), (c, up[:, :5], md, lw, ctx),
                  (c, up, md.float(), lw, ctx), (c, up, md, lw[:2], ctx), (c, up, md, lw, ctx[:1]),
                  (c, up, md, lw, ctx.float()), (c, up, md, lw, ctx[:, :7]), (c, up, md, lw, ctx[0]),
                  (c, up, md, lw, None)):
        with pytest.raises(ValueError):
            signals.grid_ladder_entry(*wrong, **kw)
