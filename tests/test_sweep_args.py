"""CPU: bq_sweep_select rejects bad arguments before any launch (no device is
touched: the pointers are fake and never dereferenced, the column table is a
host array), sizes its workspace, and mirrors the class attributes."""

import ctypes

import pytest

from binquant_amd import _lib

S, T = 8, 100
FAKE = 0x10000


def _call(**kw):
    lib = _lib.load()
    a = dict(cols=_lib.ptr_array([FAKE + 64 * k for k in range(len(_lib.SW_COLUMNS))]), ld_in=T, cross=FAKE, ld_b=T,
             route=None, ld_r=0, lens=None, first=None, rank=None, S=S, T=T, t_lo=0, t_hi=T, params=None,
             status=FAKE, score=FAKE, ld_out=T, winner=FAKE, wscore=FAKE, work=FAKE)
    a.update(kw)
    return lib.bq_sweep_select(a["cols"], a["ld_in"], a["cross"], a["ld_b"], a["route"], a["ld_r"], a["lens"],
                               a["first"], a["rank"], a["S"], a["T"], a["t_lo"], a["t_hi"], a["params"], a["status"],
                               a["score"], a["ld_out"], a["winner"], a["wscore"], a["work"], ctypes.c_void_p())


def _params(**kw):
    p = _lib.BqSweepParams()
    _lib.load().bq_sweep_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_default_params_are_the_class_attributes():
    p = _lib.BqSweepParams()
    _lib.load().bq_sweep_default_params(ctypes.byref(p))
    assert (p.min_momentum_atr, p.max_momentum_atr, p.min_close_location, p.min_frame) == (0.75, 3.0, 0.70, 56)
    assert ctypes.sizeof(_lib.BqSweepParams) == 32
    assert len(_lib.SW_COLUMNS) == 13 and len(_lib.SW_REASONS) == 15


@pytest.mark.parametrize("kw", [
    dict(cols=None), dict(cols=_lib.ptr_array([FAKE] * 12 + [0])), dict(cols=_lib.ptr_array([0] + [FAKE] * 12)),
    dict(cross=None), dict(status=None), dict(winner=None), dict(work=None), dict(work=FAKE + 4),
    dict(ld_in=T - 1), dict(ld_b=T - 1), dict(ld_out=T - 1), dict(route=FAKE, ld_r=T - 1), dict(route=FAKE, ld_r=0),
    dict(t_lo=-1), dict(t_hi=T + 1), dict(t_lo=5, t_hi=4), dict(S=-1), dict(T=-1),
    dict(S=0x80000000), dict(T=0x80000000, ld_in=0x80000000, ld_b=0x80000000, ld_out=0x80000000, t_hi=1),
], ids=lambda kw: ",".join(kw))
def test_invalid_arguments(kw):
    assert _call(**kw) == _lib.BQ_EINVAL


@pytest.mark.parametrize("kw", [dict(min_momentum_atr=float("nan")), dict(max_momentum_atr=float("inf")),
                                dict(min_close_location=float("-inf")),
                                dict(min_momentum_atr=3.5, max_momentum_atr=3.0)], ids=lambda kw: ",".join(kw))
def test_invalid_params(kw):
    assert _call(params=_params(**kw)) == _lib.BQ_EINVAL


def test_empty_problems_return_ok_without_a_launch():
    assert _call(S=0) == _lib.BQ_OK
    assert _call(T=0, t_hi=0) == _lib.BQ_OK
    assert _call(t_lo=7, t_hi=7) == _lib.BQ_OK
    assert _call(t_lo=T, t_hi=T, route=None, ld_r=0, score=None, wscore=None) == _lib.BQ_OK
    assert _call(S=0, cols=None) == _lib.BQ_EINVAL   # the checks come first


def test_workspace_size():
    ws = _lib.load().bq_sweep_select_workspace
    assert ws(0, 10) == 0 and ws(10, 0) == 0
    # 16 bytes per (row chunk, column); a narrow range's workgroups never need more
    assert ws(1, 1) == 16 and ws(64, 10) == 160 and ws(65, 10) == 320 and ws(12_500, 2_000) == 16 * 196 * 2_000
    for s in (1, 63, 64, 65, 255, 256, 257, 10_000):
        assert ws(s, 63) >= 16 * ((s + 255) // 256) * 63
