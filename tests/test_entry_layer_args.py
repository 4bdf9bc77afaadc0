"""The ValueError texts of the panel entries that share engine.py's argument
layer (impulse_rider, bb_stable, top_gainer_entry, sweep_select, retest_replay,
spike_frames, spike_fade_replay): one bad input per check, the whole message
written out. Host tensors with the native library refused wherever the check
comes before any device work; the checks that only device operands reach (a
host flag panel beside device columns, sweep_select's lens behind its flags)
are the GPU cases at the end."""

import pytest
import torch

S, T = 3, 30


@pytest.fixture
def no_library(monkeypatch):
    """The wrappers must raise before the native library is loaded."""
    from binquant_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the native library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)


def raises(message, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def f64(dev="cpu"):
    return torch.ones((S, T), dtype=torch.float64, device=dev)


def times(dev="cpu"):
    return (900_000 * torch.arange(T, dtype=torch.int64, device=dev)).expand(S, T).contiguous()


def flag(dev="cpu"):
    return torch.ones((S, T), dtype=torch.bool, device=dev)


def swapped(args, i, x):
    return [*args[:i], x, *args[i + 1:]]


def check_rows(fn, args, names=("lens", "first_t"), **kw):
    """lens / first_t / from_t: S integers."""
    for name in names:
        raises(f"{name}: expected {S} entries, got 2", fn, *args, **kw, **{name: [1, 2]})
        raises(f"{name}: expected {S} entries, got 4", fn, *args, **kw, **{name: torch.zeros(4, dtype=torch.int32)})
        raises(f"{name}: expected an integer tensor, got torch.float32", fn, *args, **kw, **{name: torch.zeros(S)})


def test_impulse_rider(no_library):
    from binquant_amd.engine import impulse_rider as fn

    a = [f64(), f64(), f64(), f64(), f64(), times(), times()[0].clone(), torch.ones(T, dtype=torch.float64)]
    raises("impulse_rider: unknown thresholds ['min_impulze'] (known: ['entry_factor', 'max_atr_pct', "
           "'max_btc_return', 'max_impulse', 'min_close_location', 'min_conf_return', 'min_history', 'min_impulse', "
           "'min_rs'])", fn, *a, min_impulze=0.1)
    raises("impulse_rider: unknown columns ['atr', 'rs']", fn, *a, columns=("atr", "atr_pct", "rs"))
    raises("close: expected [S, T] with unit stride along T", fn, *swapped(a, 3, f64()[0]))
    raises("close: expected [S, T] with unit stride along T", fn, *swapped(a, 3, None))
    raises("atr: expected dtype float64, got torch.float32", fn, *swapped(a, 4, f64().float()))
    raises("open: expected dtype float64, got <class 'list'>", fn, *swapped(a, 0, [1.0]))
    raises("low: shape (3, 29) != (3, 30)", fn, *swapped(a, 2, f64()[:, :-1]))
    raises("open_time: expected an int64 tensor of shape (3, 30)", fn, *swapped(a, 5, times().int()))
    raises("open_time: expected an int64 tensor of shape (3, 30)", fn, *swapped(a, 5, times()[:2]))
    check_rows(fn, a)


def test_bb_stable(no_library):
    from binquant_amd.engine import bb_stable as fn

    a = [f64(), f64(), f64()]
    raises("bb_mid: expected [S, T] with unit stride along T", fn, *swapped(a, 1, f64()[0]))
    raises("bb_upper: expected dtype float64, got torch.float32", fn, *swapped(a, 0, f64().float()))
    raises("bb_lower: shape (2, 30) != (3, 30)", fn, *swapped(a, 2, f64()[:2]))
    check_rows(fn, a)


def test_top_gainer_entry(no_library):
    from binquant_amd.engine import top_gainer_entry as fn

    a = [f64(), f64(), f64(), f64(), f64()]
    raises("top_gainer_entry: unknown thresholds ['min_volume'] (known: ['atr_stop_mult', 'full_extension_bars', "
           "'lookback_high', 'max_candle_return', 'max_extension', 'max_return_1h', 'max_stop_loss_pct', "
           "'max_upper_wick', 'min_candle_return', 'min_history', 'min_range_position', 'min_return_1h', "
           "'min_return_2h', 'min_return_6h', 'min_short_extension_cap', 'min_stop_loss_pct', 'min_volume_ratio', "
           "'volume_window'])", fn, *a, min_volume=1.0)
    raises("top_gainer_entry: unknown columns ['rsi']", fn, *a, columns=("ema20", "rsi"))
    raises("close: expected [S, T] with unit stride along T", fn, *swapped(a, 3, f64()[0]))
    raises("volume: expected dtype float64, got torch.float32", fn, *swapped(a, 4, f64().float()))
    raises("quote_volume: shape (3, 29) != (3, 30)", fn, *a, f64()[:, :-1])
    raises("atr: expected dtype float64, got torch.int64", fn, *a, None, times())
    raises("risk_ok: expected a bool tensor of shape (3, 30)", fn, *a, risk_ok=flag().to(torch.uint8))
    raises("risk_ok: expected a bool tensor of shape (3, 30)", fn, *a, risk_ok=flag()[:, 1:])
    check_rows(fn, a, risk_ok=flag())


def test_sweep_select(no_library):
    from binquant_amd.engine import sweep_select as fn

    cols = [f64() for _ in range(13)]
    raises("sweep_select: unknown thresholds ['min_score'] (known: ['max_momentum_atr', 'min_close_location', "
           "'min_frame', 'min_momentum_atr'])", fn, cols, flag(), min_score=1.0)
    raises("pump_score: expected [S, T] with unit stride along T", fn, swapped(cols, 0, f64()[0]), flag())
    raises("ema20: expected dtype float64, got torch.float32", fn, swapped(cols, 9, f64().float()), flag())
    raises("btc_trend_score: shape (3, 31) != (3, 30)", fn, swapped(cols, 12, torch.ones(S, T + 1).double()), flag())
    raises("score_cross: expected a bool tensor of shape (3, 30)", fn, cols, flag().to(torch.uint8))
    raises("score_cross: expected a bool tensor of shape (3, 30)", fn, cols, flag()[:2])
    raises("score_cross: expected a CUDA tensor (no CPU path)", fn, cols, flag())
    # the flags are checked one after the other: score_cross on the host comes before a malformed route_ok
    raises("score_cross: expected a CUDA tensor (no CPU path)", fn, cols, flag(), route_ok=f64())


def test_retest_replay(no_library):
    from binquant_amd.engine import retest_replay as fn

    a = [f64(), f64(), f64(), f64(), f64(), times(), flag()]
    raises("retest_replay: unknown parameters ['no_such'] (known: ['breakout_lookback', 'min_history', "
           "'pullback_factor', 'support_factor', 'watch_ms'])", fn, *a, no_such=1)
    raises("close: expected [S, T] with unit stride along T", fn, *swapped(a, 3, f64()[0]))
    raises("ema: expected dtype float64, got torch.float32", fn, *swapped(a, 4, f64().float()))
    raises("high: shape (3, 29) != (3, 30)", fn, *swapped(a, 1, f64()[:, :-1]))
    raises("open_time: expected an int64 tensor of shape (3, 30)", fn, *swapped(a, 5, times().double()))
    raises("leader: expected a bool tensor of shape (3, 30)", fn, *swapped(a, 6, flag().to(torch.uint8)))
    raises("leader: expected a bool tensor of shape (3, 30)", fn, *swapped(a, 6, flag()[:1]))
    raises("risk_ok: expected a bool tensor of shape (3, 30)", fn, *a, flag().float())
    raises("risk_ok: expected a bool tensor of shape (3, 30)", fn, *a, flag().t())
    check_rows(fn, a, ("lens", "first_t", "from_t"))


def frame_columns(dev="cpu"):
    from binquant_amd import _lib

    return {**{k: f64(dev) for k in _lib.SPIKE_FRAMES_IN}, **{k: flag(dev) for k in _lib.SPIKE_FRAMES_IN_B}}


def test_spike_frames(no_library):
    from binquant_amd import strategies
    from binquant_amd.engine import spike_frames as fn

    c, p = frame_columns(), strategies.SpikeParams()
    raises("spike_frames: unknown columns ['rsi'] (known: ('label', 'label_pre', 'label_short', 'label_short_pre', "
           "'volume_cluster_flag', 'price_break_flag', 'cumulative_price_break_flag', "
           "'cumulative_price_break_short_flag', 'accel_spike_flag', 'accel_spike_short_flag', 'upward', 'downward', "
           "'volume_cluster_min_ratio', 'price_break_base_threshold'))", fn, c, p, columns=("label", "rsi"))
    raises("close: expected [S, T] with unit stride along T", fn, {**c, "close": f64()[0]}, p)
    raises("cum_pos: expected dtype float64, got torch.float32", fn, {**c, "cum_pos": f64().float()}, p)
    raises("dyn_threshold: shape (3, 29) != (3, 30)", fn, {**c, "dyn_threshold": f64()[:, :-1]}, p)
    raises("upward: expected a bool tensor of shape (3, 30)", fn, {**c, "upward": f64()}, p)
    raises("accel_spike_flag: expected a bool tensor of shape (3, 30)", fn, {**c, "accel_spike_flag": flag()[:2]}, p)
    check_rows(fn, (c, p), ("lens", "first_t", "from_t"))
    raises("volume_ratio: expected a float64 CUDA tensor (no CPU path)", fn,
           {**c, "downward": flag().to(torch.uint8)}, p)   # uint8 flags are taken


def test_spike_fade_replay(no_library):
    from binquant_amd.engine import spike_fade_replay as fn

    a = [f64(), f64(), f64(), times(), flag()]
    raises("spike_fade_replay: unknown parameters ['window'] (known: ['ext_factor', 'window_bars'])", fn, *a, window=8)
    raises("close: expected [S, T] with unit stride along T", fn, *swapped(a, 2, f64()[0]))
    raises("high: expected dtype float64, got torch.float32", fn, *swapped(a, 1, f64().float()))
    raises("open: shape (3, 29) != (3, 30)", fn, *swapped(a, 0, f64()[:, :-1]))
    raises("open_time: expected an int64 tensor of shape (3, 30)", fn, *swapped(a, 3, times()[:, :-1]))
    raises("source_ok: expected a bool tensor of shape (3, 30)", fn, *swapped(a, 4, flag().to(torch.uint8)))
    raises("source_ok: expected a bool tensor of shape (3, 30)", fn, *swapped(a, 4, flag()[0]))
    raises("src_market: expected a bool tensor of shape (3, 30) or (30,)", fn, *a, flag().to(torch.uint8))
    raises("fail_market: expected a bool tensor of shape (3, 30) or (30,)", fn, *a, None, flag()[:, 0])
    raises("src_market / fail_market: both [S, T] or both [T] (they share one row stride)", fn, *a, flag(), flag()[0])
    check_rows(fn, a, ("lens", "first_t", "from_t"))


# ---- checks that only device operands reach ---------------------------------------

@pytest.fixture
def no_launch(monkeypatch, cuda):
    from binquant_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the native library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", refuse)
    return "cuda"


@pytest.mark.gpu
def test_host_flags_beside_device_columns(no_launch):
    from binquant_amd import engine, strategies

    d = no_launch
    five = [f64(d) for _ in range(5)]
    raises("risk_ok: expected a CUDA tensor (no CPU path)", engine.top_gainer_entry, *five, risk_ok=flag())
    cols = [f64(d) for _ in range(13)]
    raises("route_ok: expected a CUDA tensor (no CPU path)", engine.sweep_select, cols, flag(d), route_ok=flag())
    raises("leader / risk_ok / state: expected CUDA tensors (no CPU path)", engine.retest_replay, *five, times(d),
           flag())
    raises("leader / risk_ok / state: expected CUDA tensors (no CPU path)", engine.retest_replay, *five, times(d),
           flag(d), flag())
    raises("spike_frames: flag inputs: expected CUDA tensors (no CPU path)", engine.spike_frames,
           {**frame_columns(d), "upward": flag()}, strategies.SpikeParams())
    three = five[:3]
    msg = "source_ok / src_market / fail_market / state: expected CUDA tensors (no CPU path)"
    raises(msg, engine.spike_fade_replay, *three, times(d), flag())
    raises(msg, engine.spike_fade_replay, *three, times(d), flag(d), flag(d), flag())
    raises(msg, engine.spike_fade_replay, *three, times(d), flag(d), flag()[0], flag(d)[0])


@pytest.mark.gpu
def test_sweep_rows_behind_device_flags(no_launch):
    """sweep_select checks its flags' placement before lens / first_t: those two need device flags."""
    from binquant_amd.engine import sweep_select as fn

    check_rows(lambda **kw: fn([f64() for _ in range(13)], flag(no_launch), **kw), ())
