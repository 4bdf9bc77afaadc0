"""Argument checks of the per-frame failed-spike entry points that need no
device: engine.spike_frames, strategies.failed_spike_frames,
signals.spike_source_frames and the C entry bq_spike_frames reject bad input
before any device work."""

import ctypes
import dataclasses

import pytest
import torch

from binquant_amd import _lib, engine, signals, strategies


def panels(S=2, T=40, dtype=torch.float64):
    return [torch.ones((S, T), dtype=dtype) for _ in range(6)]


def cols(S=2, T=40):
    d = {k: torch.ones((S, T), dtype=torch.float64) for k in _lib.SPIKE_FRAMES_IN}
    d.update({k: torch.zeros((S, T), dtype=torch.bool) for k in _lib.SPIKE_FRAMES_IN_B})
    return d


def params(**kw):
    return dataclasses.replace(strategies.SpikeParams(), **kw)


def test_names_and_caps_match_the_header():
    assert strategies.SPIKE_FRAME_KEYS == _lib.SPIKE_FRAMES_OUT + ("volume_cluster_min_ratio",
                                                                  "price_break_base_threshold", "close_open_ratio")
    assert engine.SPIKE_FRAMES_MAX_T == 2048 >= 5 * 400   # five times the live store's frame cap
    lib = _lib.load()
    p = _lib.BqSpikeFramesParams()
    lib.bq_spike_frames_default_params(ctypes.byref(p))
    d = strategies.SpikeParams()
    want = engine.spike_frames_params(d)
    for name, _ in _lib.BqSpikeFramesParams._fields_:
        assert getattr(p, name) == getattr(want, name), name
    assert ctypes.sizeof(_lib.BqSpikeFramesParams) == 8 * 4 + 8 * 8
    assert lib.bq_spike_frames_workspace(3, 100) == 3 * 100 * 16 + 3 * 8
    assert lib.bq_spike_frames_workspace(0, 100) == 0


@pytest.mark.parametrize("bad", [dict(post_spike_cooldown_bars=64), dict(volume_cluster_window=31),
                                 dict(cumulative_price_window=31), dict(cumulative_price_window=1),
                                 dict(volume_cluster_window=0), dict(volume_cluster_label_mode="middle"),
                                 dict(volume_quantile=1.5), dict(min_volume_ratio=float("nan")),
                                 dict(base_window=31), dict(streak_length=31), dict(accel_volume_deriv_window=31),
                                 dict(price_break_use_dynamic=False)])
def test_parameters_outside_the_kernel_range(bad):
    with pytest.raises(ValueError, match="|".join(bad)):
        strategies.failed_spike_frames(*panels(), params(**bad))
    if not set(bad) & {"base_window", "streak_length", "accel_volume_deriv_window", "price_break_use_dynamic"}:
        with pytest.raises(ValueError, match="|".join(bad)):
            engine.spike_frames(cols(), params(**bad))


def test_cooldown_below_the_cap_and_disabled_pass_the_parameter_check():
    for bars in (63, 0, -1):
        assert engine.spike_frames_params(params(post_spike_cooldown_bars=bars)).post_spike_cooldown_bars == bars


def test_wrong_dtype_shape_and_columns():
    with pytest.raises(ValueError, match="float64"):
        strategies.failed_spike_frames(*panels(dtype=torch.float32))
    bad = panels()
    bad[4] = torch.ones((2, 41), dtype=torch.float64)
    with pytest.raises(ValueError, match="volume: shape"):
        strategies.failed_spike_frames(*bad)
    with pytest.raises(ValueError, match="expected \\[S, T\\]"):
        strategies.failed_spike_frames(*[x[0] for x in panels()])
    with pytest.raises(ValueError, match="unknown columns"):
        strategies.failed_spike_frames(*panels(), columns=("label", "suppressed_label"))
    with pytest.raises(ValueError, match="unknown columns"):
        engine.spike_frames(cols(), params(), columns=("close_open_ratio",))
    c = cols()
    c["dyn_threshold"] = c["dyn_threshold"].float()
    with pytest.raises(ValueError, match="dyn_threshold: expected dtype float64"):
        engine.spike_frames(c, params())
    c = cols()
    c["upward"] = c["upward"].double()
    with pytest.raises(ValueError, match="upward: expected a bool tensor"):
        engine.spike_frames(c, params())
    c = cols()
    del c["cum_neg"]
    with pytest.raises(ValueError, match="missing input columns \\['cum_neg'\\]"):
        engine.spike_frames(c, params())
    with pytest.raises(ValueError, match="first_t: expected 2 entries"):
        strategies.failed_spike_frames(*panels(), first_t=[0, 1, 2])
    with pytest.raises(ValueError, match="lens: expected an integer tensor"):
        engine.spike_frames(cols(), params(), lens=torch.ones(2))


def test_frame_over_the_cap_names_it():
    T = engine.SPIKE_FRAMES_MAX_T + 1
    with pytest.raises(ValueError, match="cap of 2048 candles"):
        strategies.failed_spike_frames(*panels(1, T))
    with pytest.raises(ValueError, match="cap of 2048 candles"):
        engine.spike_frames(cols(1, T), params())
    with pytest.raises(ValueError, match="cap of 2048 candles"):
        signals.spike_source_frames(*panels(1, T))


def test_no_cpu_path():
    with pytest.raises(ValueError, match="no CPU path"):
        strategies.failed_spike_frames(*panels())
    with pytest.raises(ValueError, match="no CPU path"):
        engine.spike_frames(cols(), params())


def test_c_entry_rejects_before_any_launch():
    lib = _lib.load()
    null = ctypes.c_void_p()
    fake = _lib.ptr_array([0x1000] * len(_lib.SPIKE_FRAMES_IN))   # never dereferenced
    fake_b = _lib.ptr_array([0x1000] * len(_lib.SPIKE_FRAMES_IN_B))
    outs = _lib.ptr_array([0] * len(_lib.SPIKE_FRAMES_OUT))

    def call(S=1, T=64, ld=64, p=None, ins=fake, ws=0x1000, ws_bytes=1 << 20):
        return lib.bq_spike_frames(ins, ld, fake_b, ld, 0, null, null, null, S, T,
                                   ctypes.byref(p) if p is not None else None, ctypes.c_void_p(ws), ws_bytes, null,
                                   null, outs, ld, null)

    assert call(ins=None) == _lib.BQ_EINVAL
    assert call(T=_lib.SPIKE_FRAMES_MAX_T + 1, ld=4096) == _lib.BQ_EINVAL
    assert call(ld=63) == _lib.BQ_EINVAL
    assert call(ws=0) == _lib.BQ_EINVAL and call(ws_bytes=64) == _lib.BQ_EINVAL and call(ws=0x1004) == _lib.BQ_EINVAL
    some_null = _lib.ptr_array([0x1000] * (len(_lib.SPIKE_FRAMES_IN) - 1) + [0])
    assert call(ins=some_null) == _lib.BQ_EINVAL
    for field, value in (("post_spike_cooldown_bars", 64), ("volume_cluster_window", 31),
                         ("cumulative_price_window", 1), ("label_mode", 3), ("volume_quantile", 1.5),
                         ("body_size_pct_min", float("inf"))):
        p = engine.spike_frames_params(strategies.SpikeParams())
        setattr(p, field, value)
        assert call(p=p) == _lib.BQ_EINVAL, field
    assert call(S=0) == _lib.BQ_OK and call(T=0) == _lib.BQ_OK   # nothing to do: no launch
