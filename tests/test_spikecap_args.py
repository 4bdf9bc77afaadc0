"""Argument checks of the frame_cap keyword that need no device:
engine.spike_frames, strategies.failed_spike_frames, signals.spike_source_frames
and the C entry bq_spike_frames_capped reject bad input before any device
work; a cap lifts the T <= 2048 limit and the uncapped call keeps its text."""

import ctypes
import dataclasses

import pytest
import torch

from binquant_amd import _lib, engine, signals, strategies


def panels(S=2, T=100, dtype=torch.float64):
    return [torch.ones((S, T), dtype=dtype) for _ in range(6)]


def cols(S=2, T=100):
    d = {k: torch.ones((S, T), dtype=torch.float64) for k in _lib.SPIKE_FRAMES_IN}
    d.update({k: torch.zeros((S, T), dtype=torch.bool) for k in _lib.SPIKE_FRAMES_IN_B})
    d.update({k: torch.zeros((S, T), dtype=torch.int32) for k in _lib.SPIKE_FRAMES_IN_I})
    return d


def params(**kw):
    return dataclasses.replace(strategies.SpikeParams(), **kw)


def raises(text, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == text


def test_names_and_struct_match_the_header():
    assert _lib.SPIKE_FRAMES_IN_I == ("dyn_src", "close_next") and _lib.SPIKE_FRAMES_MIN_CAP == 64
    assert ctypes.sizeof(_lib.BqSpikeFramesCap) == 4 * 4 + 8
    c = engine.spike_frames_cap(params(base_window=7, accel_volume_deriv_window=5, price_break_dynamic_q=0.9), 301)
    assert (c.frame_cap, c.base_window, c.accel_volume_deriv_window, c.price_break_dynamic_q) == (301, 7, 5, 0.9)
    lib = _lib.load()
    assert lib.bq_spike_frames_capped_workspace(3, 100) == 3 * 100 * 16 + 3 * 100 * 2
    assert lib.bq_spike_frames_capped_workspace(1, 3) == 3 * 16 + 8   # the byte flags padded to 8
    assert lib.bq_spike_frames_capped_workspace(0, 100) == 0


@pytest.mark.parametrize("cap", [63, 0, -1, 2049, 64.0, "301", True])
def test_cap_out_of_range_names_the_range(cap):
    text = f"spike_frames: frame_cap must be an int in 64..2048 (or None: no cap), got {cap!r}"
    raises(text, engine.spike_frames, cols(), params(), frame_cap=cap)
    raises(text, strategies.failed_spike_frames, *panels(), frame_cap=cap)
    raises(text, signals.spike_source_frames, *panels(), frame_cap=cap)


def test_cap_lifts_the_limit_on_T_and_the_uncapped_text_stays():
    T = engine.SPIKE_FRAMES_MAX_T + 1
    old = f"T = {T} exceeds the cap of 2048 candles per row"
    raises("failed_spike_frames: " + old, strategies.failed_spike_frames, *panels(1, T))
    raises("spike_frames: " + old, engine.spike_frames, cols(1, T), params())
    raises("failed_spike_frames: " + old, signals.spike_source_frames, *panels(1, T))
    # with a cap the same panels pass the argument layer and stop at the device check
    raises("open: expected a float64 CUDA tensor (no CPU path)", strategies.failed_spike_frames, *panels(1, T),
           frame_cap=64)
    raises("open: expected a float64 CUDA tensor (no CPU path)", signals.spike_source_frames, *panels(1, T),
           frame_cap=2048)
    raises("volume_ratio: expected a float64 CUDA tensor (no CPU path)", engine.spike_frames, cols(1, T), params(),
           frame_cap=301)


def test_cap_at_least_T_is_the_uncapped_call():
    """No frame slides: the index columns are not asked for."""
    c = cols(2, 100)
    for k in _lib.SPIKE_FRAMES_IN_I:
        del c[k]
    raises("volume_ratio: expected a float64 CUDA tensor (no CPU path)", engine.spike_frames, c, params(),
           frame_cap=100)
    raises("spike_frames: missing input columns ['dyn_src', 'close_next'] (frame_cap needs them)",
           engine.spike_frames, c, params(), frame_cap=99)


def test_wrong_dtype_and_shape_of_the_index_columns():
    c = cols()
    c["dyn_src"] = c["dyn_src"].long()
    raises("dyn_src: expected dtype int32, got torch.int64", engine.spike_frames, c, params(), frame_cap=64)
    c = cols()
    c["close_next"] = torch.zeros((2, 101), dtype=torch.int32)
    raises("close_next: shape (2, 101) != (2, 100)", engine.spike_frames, c, params(), frame_cap=64)
    c = cols()
    c["cum_pos"] = c["cum_pos"].float()
    raises("cum_pos: expected dtype float64, got torch.float32", engine.spike_frames, c, params(), frame_cap=64)
    bad = panels()
    bad[4] = torch.ones((2, 99), dtype=torch.float64)
    raises("volume: shape (2, 99) != (2, 100)", strategies.failed_spike_frames, *bad, frame_cap=64)
    raises("spike_frames: base_window and accel_volume_deriv_window must be in 1..30 under a frame_cap, got (31, 3)",
           engine.spike_frames, cols(), params(base_window=31), frame_cap=64)
    raises("spike_frames: price_break_dynamic_q must lie in [0, 1], got 1.5", engine.spike_frames, cols(),
           params(price_break_dynamic_q=1.5), frame_cap=64)


def test_c_entry_rejects_before_any_launch():
    lib = _lib.load()
    null = ctypes.c_void_p()
    fake = _lib.ptr_array([0x1000] * len(_lib.SPIKE_FRAMES_IN))   # never dereferenced
    fake_b = _lib.ptr_array([0x1000] * len(_lib.SPIKE_FRAMES_IN_B))
    fake_i = _lib.ptr_array([0x1000] * len(_lib.SPIKE_FRAMES_IN_I))
    outs = _lib.ptr_array([0] * len(_lib.SPIKE_FRAMES_OUT))
    good = dict(frame_cap=64, base_window=12, accel_volume_deriv_window=3, price_break_dynamic_q=0.85)

    def call(S=1, T=128, ld=128, ld_i=None, ins=fake, ins_i=fake_i, ws=0x1000, ws_bytes=1 << 20, cap=good, p=None):
        c = None
        if cap is not None:
            c = ctypes.byref(_lib.BqSpikeFramesCap(cap["frame_cap"], cap["base_window"],
                                                   cap["accel_volume_deriv_window"], 0,
                                                   cap["price_break_dynamic_q"]))
        return lib.bq_spike_frames_capped(ins, ld, fake_b, ld, ins_i, ld if ld_i is None else ld_i, 0, null, null,
                                          null, S, T, ctypes.byref(p) if p is not None else None, c,
                                          ctypes.c_void_p(ws), ws_bytes, null, null, outs, ld, null)

    assert call(S=0) == _lib.BQ_OK and call(T=0) == _lib.BQ_OK   # nothing to do: no launch
    assert call(S=0, T=4096, ld=4096) == _lib.BQ_OK              # T past BQ_SPIKE_FRAMES_MAX_T is in range
    assert call(cap=None) == _lib.BQ_EINVAL
    for k, values in (("frame_cap", (63, 0, 2049)), ("base_window", (0, 31)),
                      ("accel_volume_deriv_window", (0, 31)), ("price_break_dynamic_q", (-0.1, 1.5, float("nan")))):
        for x in values:
            assert call(cap={**good, k: x}) == _lib.BQ_EINVAL, (k, x)
    assert call(ins_i=None) == _lib.BQ_EINVAL
    assert call(ins_i=_lib.ptr_array([0x1000, 0])) == _lib.BQ_EINVAL
    assert call(ld_i=127) == _lib.BQ_EINVAL and call(ld=127) == _lib.BQ_EINVAL
    assert call(ins=None) == _lib.BQ_EINVAL
    assert call(T=(1 << 30) + 1, ld=(1 << 30) + 1) == _lib.BQ_EINVAL
    assert call(ws=0) == _lib.BQ_EINVAL and call(ws_bytes=64) == _lib.BQ_EINVAL and call(ws=0x1004) == _lib.BQ_EINVAL
    p = engine.spike_frames_params(strategies.SpikeParams())
    p.post_spike_cooldown_bars = 64
    assert call(p=p) == _lib.BQ_EINVAL
