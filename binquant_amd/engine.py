"""Batched device entry points over the C ABI (torch tensors in, torch tensors out).

All tensors are float64 CUDA (HIP) tensors shaped [S, T] with unit stride
along T (any row stride). Launches go on torch's current stream, so results
are ordered with surrounding torch work and can be timed with torch events.
There is no CPU path: non-CUDA input raises.
"""

from __future__ import annotations

import contextlib
import ctypes
import functools
import math
from dataclasses import dataclass, field

import torch

from . import _lib
from ._lib import ENRICH_COLUMNS, FEATURE_COLUMNS, INPUT_FIELDS, PARTIAL_COLUMNS


@dataclass
class IndicatorParams:
    """Python mirror of ``bq_params``; defaults are the reference's windows
    (producers/context_evaluator.py:249-261)."""

    ma_periods: tuple[int, int, int] = (7, 25, 100)
    macd_fast: int = 12
    macd_slow: int = 26
    macd_signal: int = 9
    rsi_window: int = 14
    bb_window: int = 20
    bb_ddof: int = 1
    bb_k: float = 2.0
    atr_window: int = 14
    twap_window: int = 12
    ema_spans: tuple[int, int] = (20, 50)
    mfi_window: int = 14
    extra: dict = field(default_factory=dict)

    def to_c(self) -> _lib.BqParams:
        p = _lib.BqParams()
        for i, v in enumerate(self.ma_periods):
            p.ma_periods[i] = int(v)
        p.macd_fast = int(self.macd_fast)
        p.macd_slow = int(self.macd_slow)
        p.macd_signal = int(self.macd_signal)
        p.rsi_window = int(self.rsi_window)
        p.bb_window = int(self.bb_window)
        p.bb_ddof = int(self.bb_ddof)
        p.atr_window = int(self.atr_window)
        p.twap_window = int(self.twap_window)
        p.ema_spans[0] = int(self.ema_spans[0])
        p.ema_spans[1] = int(self.ema_spans[1])
        p.mfi_window = int(self.mfi_window)
        p.bb_k = float(self.bb_k)
        return p

    def as_oracle_dict(self) -> dict:
        return dict(
            ma_periods=tuple(self.ma_periods),
            macd_fast=self.macd_fast,
            macd_slow=self.macd_slow,
            macd_signal=self.macd_signal,
            rsi_window=self.rsi_window,
            bb_window=self.bb_window,
            bb_ddof=self.bb_ddof,
            bb_k=self.bb_k,
            atr_window=self.atr_window,
            twap_window=self.twap_window,
            ema_spans=tuple(self.ema_spans),
            mfi_window=self.mfi_window,
        )


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_handle(stream: torch.cuda.Stream | None) -> ctypes.c_void_p:
    """hipStream_t of `stream`, else of torch's current stream on the current
    device (read without building a Stream object: this runs once per launch)."""
    if stream is not None:
        return ctypes.c_void_p(stream.cuda_stream)
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_tensors(obj, out: list) -> list:
    """CUDA tensors among a call's arguments (tensors, and tensors inside
    lists / tuples / dict values one level down)."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            out.append(obj)
    elif isinstance(obj, (list, tuple)):
        # sequences of operands are homogeneous: a list whose first entry is
        # not a tensor (e.g. 10k symbol names of a store tick) is not walked
        if obj and isinstance(obj[0], torch.Tensor):
            for x in obj:
                if isinstance(x, torch.Tensor) and x.is_cuda:
                    out.append(x)
    elif isinstance(obj, dict):
        for x in obj.values():
            if isinstance(x, torch.Tensor) and x.is_cuda:
                out.append(x)
    elif isinstance(getattr(obj, "x", None), torch.Tensor) and obj.x.is_cuda:   # Roll / Ewm / Ffill specs
        out.append(obj.x)
    return out


@contextlib.contextmanager
def launch_scope(device: torch.device | None, stream: torch.cuda.Stream | None, tensors=()):
    """Where and when a native launch runs.

    * device — made current for the call: the C ABI launches on the current
      device's stream, and the fused JIT resolves its module per current device.
    * stream — when given, it first waits on the device's current stream (the
      producers of the operands), the call runs under torch.cuda.stream(stream)
      so outputs and temporaries are allocated and produced on it, and every
      CUDA operand is recorded on it so the caching allocator does not hand
      the memory out again before the stream has read it. Later use of the
      outputs on another stream is the caller's to order, as with any torch
      side stream.
    """
    if device is not None and device.type != "cuda":   # host tensors (CPU rehearsal of the collectives)
        yield
        return
    if stream is None:
        if device is None or device.index is None or device.index == (
                _cur_device() if _cur_device else torch.cuda.current_device()):
            yield
            return
        with torch.cuda.device(device):
            yield
        return
    if device is not None:
        # torch.device("cuda") (index None) means the current device
        want = device.index if device.index is not None else torch.cuda.current_device()
        have = stream.device.index if stream.device.index is not None else torch.cuda.current_device()
        if want != have:
            raise ValueError(f"stream is on {stream.device}, operands on {device}")
    with torch.cuda.device(stream.device):
        stream.wait_stream(torch.cuda.current_stream(stream.device))
        for t in tensors:
            t.record_stream(stream)
        with torch.cuda.stream(stream):
            yield


def device_entry(fn):
    """Decorator of the public entry points: runs `fn` on the device holding
    its CUDA operands (all must share one device) and, for `stream=`, under
    launch_scope's stream ordering. The wrapped body always launches on the
    current stream."""

    @functools.wraps(fn)
    def wrapper(*args, stream: torch.cuda.Stream | None = None, **kw):
        ts: list = []
        for a in args:
            _cuda_tensors(a, ts)
        for a in kw.values():
            _cuda_tensors(a, ts)
        dev = ts[0].device if ts else None
        if dev is not None:
            for t in ts:
                if t.device != dev:
                    raise ValueError(f"{fn.__name__}: operands on {dev} and {t.device}; one device per call")
        if stream is None and (dev is None or dev.index == (_cur_device() if _cur_device else -1)):
            return fn(*args, **kw)
        with launch_scope(dev, stream, ts):
            return fn(*args, **kw)

    return wrapper


def _check_panel(x: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{name}: expected a float64 CUDA tensor (no CPU path)")
    if x.dtype != torch.float64:
        raise ValueError(f"{name}: expected dtype float64, got {x.dtype}")
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{name}: expected [S, T] with unit stride along T")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(x.shape)} != {tuple(shape)}")
    return x


def _panels(tensors, names, S: int, T: int) -> list[torch.Tensor]:
    """The tensors checked against (S, T) (_check_panel), contiguous."""
    return [_check_panel(t, n, (S, T)).contiguous() for t, n in zip(tensors, names)]


def _bench_rows(T: int, **rows) -> list[torch.Tensor]:
    """The benchmark's rows (name=tensor) as contiguous [T] vectors."""
    for n, t in rows.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.numel() != T:
            raise ValueError(f"{n}: expected a float64 CUDA tensor of {T} values")
    return [t.reshape(T).contiguous() for t in rows.values()]


def _row_stride(x: torch.Tensor) -> int:
    return int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])


def _hlc_panel(high, low, close):
    """(high, low, close) checked as one [S, T] panel: ([high, low, close], S,
    T, their common row stride); columns of different strides are made
    contiguous."""
    close = _check_panel(close, "close")
    S, T = close.shape
    hlc = [_check_panel(t, n, (S, T)) for t, n in zip((high, low, close), ("high", "low", "close"))]
    ld_in = _row_stride(hlc[0])
    if any(_row_stride(t) != ld_in for t in hlc):
        hlc = [t.contiguous() for t in hlc]
        ld_in = T
    return hlc, S, T, ld_in


def _feature_columns(feats: dict[str, torch.Tensor], S: int, T: int):
    """The six [S, T] feature columns in FEATURE_COLUMNS order and their common row stride."""
    fs = [_check_panel(feats[n], n, (S, T)) for n in FEATURE_COLUMNS]
    ld_f = _row_stride(fs[0])
    if any(_row_stride(t) != ld_f for t in fs):
        raise ValueError("feature columns must share one row stride")
    return fs, ld_f


def _partial_out(out: torch.Tensor | None, T: int, device) -> torch.Tensor:
    """The [T, 10] partials tensor: the caller's, checked, or a new one."""
    if out is None:
        return torch.empty((T, len(PARTIAL_COLUMNS)), dtype=torch.float64, device=device)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == device
            and tuple(out.shape) == (T, len(PARTIAL_COLUMNS)) and out.is_contiguous()):
        raise ValueError(f"out: expected a contiguous float64 [{T}, {len(PARTIAL_COLUMNS)}] tensor on {device}")
    return out


ENRICH_ROW_PAD = 192   # doubles added to each output row's pitch by enrich_outputs (tools/shard_pitch.py)


def enrich_outputs(S: int, T: int, device, columns=ENRICH_COLUMNS) -> dict[str, torch.Tensor]:
    """Output columns for enrich(..., out=...) laid out for HBM: [S, T] views
    into [S, T + ENRICH_ROW_PAD] buffers when the panel is large. With a row
    pitch of exactly T doubles (80 000 B at T = 10 000) the concurrently
    resident workgroups' output streams meet the same HBM channels: the C4
    shard (12 500 x 10 000) ran at 0.666 of 8 TB/s, at 0.711 with a 512-B pad
    (round 5). Round 6 swept the pad on two boxes (profiles/r6d_pitch.txt,
    r6e_pitch.txt): +512 B 0.709 / 0.626, +768 B 0.719 / 0.692, +1 536 B
    0.713 / 0.702 at the shard, the 100k headline indifferent — 192 doubles.
    Small panels get plain [S, T] tensors. enrich() allocates its own outputs
    this way too."""
    pad = ENRICH_ROW_PAD if S >= 1024 and T >= 1024 else 0
    return {k: torch.empty((S, T + pad), dtype=torch.float64, device=device)[:, :T] for k in columns}


@device_entry
def enrich(
    open_: torch.Tensor,
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    volume: torch.Tensor,
    params: IndicatorParams | None = None,
    columns=ENRICH_COLUMNS,
    out: dict[str, torch.Tensor] | None = None,
    stream: torch.cuda.Stream | None = None,
) -> dict[str, torch.Tensor]:
    """Full (or partial) indicator set over a [S, T] panel in ONE kernel launch.

    Replaces ContextEvaluator.indicators_enrichment
    (producers/context_evaluator.py:240-263) applied symbol by symbol.
    Returns {column_name: [S, T] float64 tensor}.
    """
    close = _check_panel(close, "close")
    S, T = close.shape
    ins = [
        _check_panel(t, n, (S, T))
        for t, n in zip((open_, high, low, close, volume), INPUT_FIELDS)
    ]
    ld_in = _row_stride(ins[0])
    if any(_row_stride(t) != ld_in for t in ins):
        ins = [t.contiguous() for t in ins]
        ld_in = T
    cols = tuple(columns)
    unknown = set(cols) - set(ENRICH_COLUMNS)
    if unknown:
        raise ValueError(f"unknown enrich columns: {sorted(unknown)}")
    out = dict(out or {})
    given = [n for n in cols if n in out]
    for name in given:
        _check_panel(out[name], f"out[{name}]", (S, T))
    missing = [n for n in cols if n not in out]
    if missing:
        # the columns this call allocates share the caller's pitch when some
        # are given, else enrich_outputs' rule (a padded pitch on large panels:
        # the layout the bench times is the one every product caller gets)
        if given:
            ld = _row_stride(out[given[0]])
            out.update({n: torch.empty((S, max(ld, T)), dtype=torch.float64, device=close.device)[:, :T]
                        for n in missing})
        else:
            out.update(enrich_outputs(S, T, close.device, missing))
    ld_out = T
    if out:
        strides = {_row_stride(out[n]) for n in cols}
        if len(strides) != 1:
            raise ValueError("all output columns must share one row stride")
        ld_out = strides.pop()
    in_arr = _lib.ptr_array([t.data_ptr() for t in ins])
    out_arr = _lib.ptr_array([out[n].data_ptr() if n in cols else 0 for n in ENRICH_COLUMNS])
    p = (params or IndicatorParams()).to_c()
    st = _lib.load().bq_enrich(
        in_arr, S, T, ld_in, ctypes.byref(p), out_arr, ld_out, _stream_handle(stream)
    )
    _lib.check(st, "bq_enrich")
    return {n: out[n] for n in cols}


@device_entry
def market_features(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    max_bars: int = 400,
    out: dict[str, torch.Tensor] | None = None,
    stream: torch.cuda.Stream | None = None,
) -> dict[str, torch.Tensor]:
    """_compute_symbol_features at every timestamp of a [S, T] panel
    (market_regime/live_market_context_accumulator.py:244-297) under the
    MarketStateStore history cap ``max_bars`` (klines_provider.py:40,65 uses 400)."""
    hlc, S, T, ld_in = _hlc_panel(high, low, close)
    out = dict(out or {})
    for name in FEATURE_COLUMNS:
        if name not in out:
            out[name] = torch.empty((S, T), dtype=torch.float64, device=hlc[2].device)
        else:
            _check_panel(out[name], f"out[{name}]", (S, T))
    ld_out = _row_stride(out[FEATURE_COLUMNS[0]])
    if any(_row_stride(out[n]) != ld_out for n in FEATURE_COLUMNS):
        raise ValueError("all feature output columns must share one row stride")
    st = _lib.load().bq_market_features(
        _lib.ptr_array([t.data_ptr() for t in hlc]),
        S,
        T,
        ld_in,
        int(max_bars),
        _lib.ptr_array([out[n].data_ptr() for n in FEATURE_COLUMNS]),
        ld_out,
        _stream_handle(stream),
    )
    _lib.check(st, "bq_market_features")
    return out


PUMP_COLUMNS = ("candidate_atr", "momentum_3", "relative_volume", "pre_breakout_compression", "pump_score",
                "prior_high", "close_location", "ema20", "ema50", "trend_score", "momentum_atr", "btc_momentum_3",
                "btc_trend_score", "relative_strength")


@device_entry
def pump_features(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    volume: torch.Tensor,
    candidate_atr: torch.Tensor,
    ema20: torch.Tensor,
    ema50: torch.Tensor,
    bench_ffill: torch.Tensor,
    bench_ema20: torch.Tensor,
    bench_ema50: torch.Tensor,
    momentum_bars: int = 3,
    volume_lookback: int = 20,
    compression_bars: int = 6,
    stream: torch.cuda.Stream | None = None,
    trend_score: torch.Tensor | None = None,
) -> dict[str, torch.Tensor]:
    """LiquidationSweepPump.compute_pump_score's columns but the two rolling
    quantiles and score_cross (strategies/liquidation_sweep_pump.py:195-268) in
    one pass per row (bq_pump_features): the volume mean, the high / low
    windows and the pad-filled pct_change formed in the kernel. The ewm columns
    (candidate_atr, ema20, ema50) and the benchmark rows ([T]: ffilled close,
    ewm 20, ewm 50) are inputs; the returned ewm columns ARE those input
    tensors (the kernel does not write a copy: 24 B per candle less).
    trend_score: the column already formed with the ewm columns (bq_pump_ewm);
    then the kernel reads neither ema column back and returns it as given."""
    close = _check_panel(close, "close")
    S, T = close.shape
    ins = _panels((high, low, close, volume, candidate_atr, ema20, ema50),
                  ("high", "low", "close", "volume", "candidate_atr", "ema20", "ema50"), S, T)
    if trend_score is not None:
        trend_score = _check_panel(trend_score, "trend_score", (S, T))
    bench = _bench_rows(T, bench_ffill=bench_ffill, bench_ema20=bench_ema20, bench_ema50=bench_ema50)
    given = {"candidate_atr": ins[4], "ema20": ins[5], "ema50": ins[6]}
    if trend_score is not None:
        given["trend_score"] = trend_score
    out = {n: given[n] if n in given else torch.empty((S, T), dtype=torch.float64, device=close.device)
           for n in PUMP_COLUMNS}
    iptr = [t.data_ptr() for t in ins]
    if trend_score is not None:
        iptr[5] = iptr[6] = 0   # not read
    st = _lib.load().bq_pump_features(
        _lib.ptr_array(iptr), S, T, T, _lib.ptr_array([t.data_ptr() for t in bench]),
        int(momentum_bars), int(volume_lookback), int(compression_bars),
        _lib.ptr_array([0 if n in given else out[n].data_ptr() for n in PUMP_COLUMNS]), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_pump_features")
    return out


@device_entry
def pump_features_ewm(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    volume: torch.Tensor,
    bench_ffill: torch.Tensor,
    bench_ema20: torch.Tensor,
    bench_ema50: torch.Tensor,
    momentum_bars: int = 3,
    volume_lookback: int = 20,
    compression_bars: int = 6,
    stream: torch.cuda.Stream | None = None,
) -> dict[str, torch.Tensor]:
    """pump_features with candidate_atr / ema20 / ema50 formed inside the pass
    (bq_pump_features_ewm: the three ewm scans on the row's tiles, no ewm
    column read back; liquidation_sweep_pump.py:206-217, 252-253)."""
    close = _check_panel(close, "close")
    S, T = close.shape
    ins = _panels((high, low, close, volume), ("high", "low", "close", "volume"), S, T)
    bench = _bench_rows(T, bench_ffill=bench_ffill, bench_ema20=bench_ema20, bench_ema50=bench_ema50)
    out = {n: torch.empty((S, T), dtype=torch.float64, device=close.device) for n in PUMP_COLUMNS}
    st = _lib.load().bq_pump_features_ewm(
        _lib.ptr_array([t.data_ptr() for t in ins]), S, T, T, _lib.ptr_array([t.data_ptr() for t in bench]),
        int(momentum_bars), int(volume_lookback), int(compression_bars),
        _lib.ptr_array([out[n].data_ptr() for n in PUMP_COLUMNS]), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_pump_features_ewm")
    return out


@device_entry
def pump_ewm(high: torch.Tensor, low: torch.Tensor, close: torch.Tensor,
             stream: torch.cuda.Stream | None = None, trend: bool = False) -> tuple[torch.Tensor, ...]:
    """LiquidationSweepPump's candidate_atr (TR.ewm(alpha=1/14, min_periods=14))
    and ema20 / ema50 of close in panel mode, one pass per row (bq_pump_ewm:
    the true range formed in the kernel; liquidation_sweep_pump.py:206-217,
    252-253); trend=True adds trend_score = (ema20 - ema50) / ema50 (:254)."""
    close = _check_panel(close, "close").contiguous()
    S, T = close.shape
    high = _check_panel(high, "high", (S, T)).contiguous()
    low = _check_panel(low, "low", (S, T)).contiguous()
    outs = [torch.empty((S, T), dtype=torch.float64, device=close.device) for _ in range(4 if trend else 3)]
    st = _lib.load().bq_pump_ewm(_ptr(high), _ptr(low), _ptr(close), S, T, T, *(_ptr(o) for o in outs[:3]),
                                 _ptr(outs[3] if trend else None), T, _stream_handle(stream))
    _lib.check(st, "bq_pump_ewm")
    return tuple(outs)


BURST_FLOAT_COLUMNS = ("baseline_volume_safe", "volume_ratio", "baseline_quote_volume_safe", "quote_volume_ratio",
                       "price_jump", "range_frac", "body_frac", "close_to_high", "recent_up_closes",
                       "activity_burst_score")
BURST_BOOL_COLUMNS = ("is_bullish", "vol_spike", "quote_vol_spike", "price_jump_flag", "range_expansion_flag",
                      "body_quality_flag", "trend_quality_flag")


@device_entry
def burst_features(
    o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, v: torch.Tensor,
    qv: torch.Tensor | None, baseline_volume: torch.Tensor, baseline_quote_volume: torch.Tensor | None,
    params, stream: torch.cuda.Stream | None = None,
) -> tuple[dict[str, torch.Tensor], torch.Tensor]:
    """ActivityBurstPump.compute_indicators' columns of
    strategies/activity_burst_pump.py:58-133 in one pass (bq_burst_features),
    given the two baseline medians; returns (columns, the AND of the six flags
    as uint8 for burst_qualify). Without a quote volume the quote baseline and
    its safe column alias the volume's (the reference's fallback)."""
    c = _check_panel(c, "c")
    S, T = c.shape
    has_q = qv is not None
    names = ("o", "h", "l", "c", "v", "qv", "baseline_volume", "baseline_quote_volume")
    ins = []
    for t, n in zip((o, h, l, c, v, qv, baseline_volume, baseline_quote_volume), names):
        ins.append(None if t is None else _check_panel(t, n, (S, T)).contiguous())
    if has_q != (baseline_quote_volume is not None):
        raise ValueError("qv and baseline_quote_volume: give both or neither")
    out = {n: torch.empty((S, T), dtype=torch.float64, device=c.device) for n in BURST_FLOAT_COLUMNS
           if has_q or n != "baseline_quote_volume_safe"}
    flags = {n: torch.empty((S, T), dtype=torch.bool, device=c.device) for n in BURST_BOOL_COLUMNS}
    all_flags = torch.empty((S, T), dtype=torch.uint8, device=c.device)
    pr = _lib.BqBurstParams(float(params.volume_multiplier), float(params.quote_volume_multiplier),
                            float(params.price_threshold), float(params.min_baseline_volume),
                            float(params.min_range_frac), float(params.min_body_frac), float(params.max_close_to_high),
                            int(params.min_recent_up_closes if has_q else 1), 0)
    st = _lib.load().bq_burst_features(
        _lib.ptr_array([0 if t is None else t.data_ptr() for t in ins]), S, T, T, ctypes.byref(pr),
        _lib.ptr_array([out[n].data_ptr() if n in out else 0 for n in BURST_FLOAT_COLUMNS]),
        _lib.ptr_array([flags[n].data_ptr() for n in BURST_BOOL_COLUMNS]), ctypes.c_void_p(all_flags.data_ptr()), T,
        _stream_handle(stream),
    )
    _lib.check(st, "bq_burst_features")
    if not has_q:
        out["baseline_quote_volume_safe"] = out["baseline_volume_safe"]
    out.update(flags)
    return out, all_flags


@device_entry
def burst_qualify(score: torch.Tensor, threshold: torch.Tensor, all_flags: torch.Tensor, cooldown_bars: int = 3,
                  stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """qualified_signal (strategies/activity_burst_pump.py:140-156): raw = the
    six flags & (score >= threshold.fillna(0)), cleared where raw fired in the
    cooldown_bars candles before (bq_burst_qualify). bool [S, T]."""
    score = _check_panel(score, "score")
    S, T = score.shape
    threshold = _check_panel(threshold, "threshold", (S, T)).contiguous()
    score = score.contiguous()
    if not isinstance(all_flags, torch.Tensor) or all_flags.dtype != torch.uint8 or tuple(all_flags.shape) != (S, T):
        raise ValueError("all_flags: expected the uint8 [S, T] tensor of burst_features")
    all_flags = all_flags.contiguous()
    q = torch.empty((S, T), dtype=torch.bool, device=score.device)
    st = _lib.load().bq_burst_qualify(
        ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(threshold.data_ptr()), ctypes.c_void_p(all_flags.data_ptr()),
        S, T, T, T, int(cooldown_bars), ctypes.c_void_p(q.data_ptr()), _stream_handle(stream),
    )
    _lib.check(st, "bq_burst_qualify")
    return q


SPIKE_BASE_FLOAT = ("price_change", "price_change_abs", "body_size", "body_size_pct", "upper_wick", "lower_wick",
                    "upper_wick_ratio", "lower_wick_ratio", "total_range", "range_pct", "close_open_ratio", "price_ma",
                    "price_zscore", "volume_ma", "volume_ratio", "volume_zscore", "quote_volume_ma",
                    "quote_volume_ratio", "momentum_3", "momentum_5", "close_to_high", "close_to_low",
                    "std_ratio_8_20", "pc_2c", "pc_3c", "pc_pos_count_5", "pc_abs_sum_5", "body_size_pct_ma_10",
                    "body_size_pct_z")
SPIKE_BASE_BOOL = ("is_bullish", "vol_compression_flag", "upward", "downward")
SPIKE_FLAG_FLOAT = ("vol_ratio_slope_3", "vol_ratio_accel", "price_break_threshold_series", "early_spike_proba")
SPIKE_FLAG_BOOL = ("volume_cluster_flag", "price_break_flag", "cumulative_price_break_flag",
                   "cumulative_price_break_short_flag", "accel_spike_flag", "accel_spike_short_flag", "label_pre",
                   "label_short_pre", "early_proba_aug_flag")


def _cols(S, T, dev, names, dtype, given=None):
    given = given or {}
    return {n: given[n] if n in given else torch.empty((S, T), dtype=dtype, device=dev) for n in names}


# bq_spike_base_std's std columns (enum bq_spike_std_col), under their
# FailedSpikeFade.detect names
SPIKE_STD = ("price_std", "volume_std", "rolling_price_std_8", "rolling_price_std_20", "body_size_pct_std_10")


def _spike_base(entry: str, ins, names, base_window, streak_length, body_size_pct, stream) -> dict[str, torch.Tensor]:
    """spike_base / spike_base_std: ins[3] is the close; bq_spike_base_std also
    writes (and returns) the SPIKE_STD columns."""
    c = _check_panel(ins[3], "c")
    S, T = c.shape
    ins = _panels(ins, names, S, T)
    out = _cols(S, T, c.device, SPIKE_BASE_FLOAT, torch.float64,
                {"body_size_pct": body_size_pct} if body_size_pct is not None else None)
    flags = _cols(S, T, c.device, SPIKE_BASE_BOOL, torch.bool)
    sd = _cols(S, T, c.device, SPIKE_STD, torch.float64) if entry == "bq_spike_base_std" else {}
    st = getattr(_lib.load(), entry)(
        _lib.ptr_array([t.data_ptr() for t in ins]), S, T, T, int(base_window), int(streak_length),
        _lib.ptr_array([0 if (n == "body_size_pct" and body_size_pct is not None) else out[n].data_ptr()
                        for n in SPIKE_BASE_FLOAT]),
        _lib.ptr_array([flags[n].data_ptr() for n in SPIKE_BASE_BOOL]),
        *([_lib.ptr_array([sd[n].data_ptr() for n in SPIKE_STD])] if sd else []), T, _stream_handle(stream),
    )
    _lib.check(st, entry)
    out.update(flags)
    out.update(sd)
    return out


@device_entry
def spike_base(o, h, l, c, v, qv, close_ffill, price_std, volume_std, std8, std20, body_pct_std, base_window: int = 12,
               streak_length: int = 3, body_size_pct: torch.Tensor | None = None,
               stream: torch.cuda.Stream | None = None) -> dict[str, torch.Tensor]:
    """FailedSpikeFade's base and early-feature columns
    (strategies/failed_spike_fade.py:260-357) in one pass per row
    (bq_spike_base), given the ffilled close and the rolling std columns;
    body_size_pct: an existing column with the kernel's values (not rewritten)."""
    return _spike_base(
        "bq_spike_base", (o, h, l, c, v, qv, close_ffill, price_std, volume_std, std8, std20, body_pct_std),
        ("o", "h", "l", "c", "v", "qv", "close_ffill", "price_std", "volume_std", "std8", "std20", "body_pct_std"),
        base_window, streak_length, body_size_pct, stream)


@device_entry
def spike_base_std(o, h, l, c, v, qv, close_ffill, base_window: int = 12, streak_length: int = 3,
                   body_size_pct: torch.Tensor | None = None,
                   stream: torch.cuda.Stream | None = None) -> dict[str, torch.Tensor]:
    """spike_base in panel mode (bq_spike_base_std): the five rolling std
    columns (failed_spike_fade.py:293-339) formed in the same pass as two-pass
    window sums — the window's variance to rounding, where pandas' online
    recurrence (and its bit-exact replay, spike_base's inputs) drifts — and
    returned beside the base columns under their detect() names."""
    return _spike_base("bq_spike_base_std", (o, h, l, c, v, qv, close_ffill),
                       ("o", "h", "l", "c", "v", "qv", "close_ffill"), base_window, streak_length, body_size_pct,
                       stream)


_SPIKE_MODES = {"last": 0, "first": 1, "all": 2}


@device_entry
def spike_flags(o, c, close_ffill, volume_ratio, dyn_threshold, vcmr, pbbt, params,
                stream: torch.cuda.Stream | None = None, labels: torch.Tensor | None = None) -> dict[str, torch.Tensor]:
    """FailedSpikeFade's flag columns and preliminary labels
    (strategies/failed_spike_fade.py:360-488) in one pass per row
    (bq_spike_flags): vcmr / pbbt [S] the calibrated thresholds, dyn_threshold
    the |pct change| rolling quantile. labels: an optional bool [2, S, T]
    that receives label_pre / label_short_pre (so one cooldown launch can
    take both as [2S, T] rows)."""
    c = _check_panel(c, "c")
    S, T = c.shape
    ins = _panels((o, c, close_ffill, volume_ratio, dyn_threshold),
                  ("o", "c", "close_ffill", "volume_ratio", "dyn_threshold"), S, T)
    vc = vcmr.reshape(S).contiguous().to(torch.float64)
    pb = pbbt.reshape(S).contiguous().to(torch.float64)
    pr = _lib.BqSpikeParams(int(params.volume_cluster_window), int(params.volume_cluster_min_count),
                            int(params.cumulative_price_window), int(params.accel_volume_deriv_window),
                            _SPIKE_MODES[params.volume_cluster_label_mode], int(bool(params.require_both_patterns)),
                            int(bool(params.require_bullish_spike)), 0, float(params.cumulative_price_threshold),
                            float(params.accel_volume_deriv_min), float(params.accel_price_change_min),
                            float(params.body_size_pct_min))
    out = _cols(S, T, c.device, SPIKE_FLAG_FLOAT, torch.float64)
    given = None
    if labels is not None:
        if labels.shape != (2, S, T) or labels.dtype != torch.bool or not labels.is_contiguous() \
                or labels.device != c.device:
            raise ValueError("labels: expected a contiguous bool [2, S, T] tensor on the panel's device")
        given = {"label_pre": labels[0], "label_short_pre": labels[1]}
    flags = _cols(S, T, c.device, SPIKE_FLAG_BOOL, torch.bool, given)
    st = _lib.load().bq_spike_flags(
        _lib.ptr_array([t.data_ptr() for t in ins]), ctypes.c_void_p(vc.data_ptr()), ctypes.c_void_p(pb.data_ptr()),
        S, T, T, ctypes.byref(pr), _lib.ptr_array([out[n].data_ptr() for n in SPIKE_FLAG_FLOAT]),
        _lib.ptr_array([flags[n].data_ptr() for n in SPIKE_FLAG_BOOL]), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_spike_flags")
    out.update(flags)
    return out


@device_entry
def breadth_partial(
    close: torch.Tensor,
    feats: dict[str, torch.Tensor],
    out: torch.Tensor | None = None,
    stream: torch.cuda.Stream | None = None,
) -> torch.Tensor:
    """[T, 10] per-timestamp partial counts/sums over this shard's symbols
    (the reductions of _build_context, live_market_context_accumulator.py:135-163)."""
    close = _check_panel(close, "close")
    S, T = close.shape
    fs, ld_f = _feature_columns(feats, S, T)
    out = _partial_out(out, T, close.device)
    st = _lib.load().bq_breadth_partial(
        ctypes.c_void_p(close.data_ptr()),
        _lib.ptr_array([t.data_ptr() for t in fs]),
        S,
        T,
        _row_stride(close),
        ld_f,
        ctypes.c_void_p(out.data_ptr()),
        _stream_handle(stream),
    )
    _lib.check(st, "bq_breadth_partial")
    return out


@dataclass
class CompactPanel:
    """compact_panel's result: each symbol's present candles packed to the
    front of its row (what MarketStateStore would hold), and where they went."""

    high: torch.Tensor        # [S, T] packed; the tail repeats the last present candle
    low: torch.Tensor
    close: torch.Tensor
    rank: torch.Tensor        # [S, T] int32: position of candle t in the packed row, -1 where absent
    n_present: torch.Tensor   # [S] int32
    first_t: torch.Tensor     # [S] int32: first present t (T if never present)
    n_invalid: torch.Tensor   # [S] int32: candles outside the domain (non-zero only with validate=False)


@device_entry
def compact_panel(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    validate: bool = True,
    stream: torch.cuda.Stream | None = None,
) -> CompactPanel:
    """Per-symbol compaction of a [S, T] panel whose absent candles (late
    listings, halts, delistings, gaps) are NaN closes: the history
    MarketStateStore keeps (it drops a candle without a close,
    market_regime/market_state_store.py:84). A present candle has a finite
    close, high and low. validate=True reads the kernel's count of candles
    outside that domain (one sync) and raises ValueError if there are any."""
    hlc, S, T, ld_in = _hlc_panel(high, low, close)
    dev = hlc[2].device
    out = [torch.empty((S, T), dtype=torch.float64, device=dev) for _ in range(3)]
    ld_r = (T + 3) // 4 * 4   # 16-byte aligned rank rows
    rank = torch.empty((S, ld_r), dtype=torch.int32, device=dev)[:, :T]
    n_present, first_t, n_invalid = (torch.empty(S, dtype=torch.int32, device=dev) for _ in range(3))
    st = _lib.load().bq_panel_compact(
        _lib.ptr_array([t.data_ptr() for t in hlc]), S, T, ld_in,
        _lib.ptr_array([t.data_ptr() for t in out]), T,
        ctypes.c_void_p(rank.data_ptr()), ld_r,
        ctypes.c_void_p(n_present.data_ptr()), ctypes.c_void_p(first_t.data_ptr()),
        ctypes.c_void_p(n_invalid.data_ptr()), _stream_handle(stream))
    _lib.check(st, "bq_panel_compact")
    if validate and S and int(n_invalid.sum().item()):
        row = int(torch.nonzero(n_invalid)[0, 0].item())
        raise ValueError(
            f"compact_panel: row {row} holds {int(n_invalid[row].item())} candle(s) outside the panel domain "
            "(a +-inf close, or a present candle without a finite high / low); histories with candles "
            "without high or low go through DeviceMarketStateStore")
    return CompactPanel(high=out[0], low=out[1], close=out[2], rank=rank, n_present=n_present, first_t=first_t,
                        n_invalid=n_invalid)


@device_entry
def breadth_partial_fresh(
    compact: CompactPanel,
    feats: dict[str, torch.Tensor],
    out: torch.Tensor | None = None,
    stream: torch.cuda.Stream | None = None,
) -> torch.Tensor:
    """[T, 10] partials over the symbols fresh at each timestamp
    (get_fresh_symbols, market_regime/market_state_store.py:49-54, into the
    reductions of _build_context, live_market_context_accumulator.py:135-163).
    feats = market_features on the compacted panel. Column 9 is the shard's
    tracked count at t (symbols listed at or before t)."""
    close = _check_panel(compact.close, "compact.close")
    S, T = close.shape
    fs, ld_f = _feature_columns(feats, S, T)
    rank, first_t = compact.rank, compact.first_t
    if not (rank.is_cuda and rank.dtype == torch.int32 and tuple(rank.shape) == (S, T)
            and (T <= 1 or rank.stride(1) == 1)):
        raise ValueError(f"compact.rank: expected an int32 CUDA [{S}, {T}] tensor with unit stride along T")
    if not (first_t.is_cuda and first_t.dtype == torch.int32 and tuple(first_t.shape) == (S,)
            and first_t.is_contiguous()):
        raise ValueError(f"compact.first_t: expected a contiguous int32 CUDA [{S}] tensor")
    out = _partial_out(out, T, close.device)
    st = _lib.load().bq_breadth_partial_fresh(
        ctypes.c_void_p(close.data_ptr()),
        _lib.ptr_array([t.data_ptr() for t in fs]),
        ctypes.c_void_p(rank.data_ptr()),
        ctypes.c_void_p(first_t.data_ptr()),
        S, T, _row_stride(close), ld_f, _row_stride(rank),
        ctypes.c_void_p(out.data_ptr()),
        _stream_handle(stream),
    )
    _lib.check(st, "bq_breadth_partial_fresh")
    return out


REGIME_PANEL_COLUMNS = _lib.REGIME_PANEL_COLUMNS


def _panel_index(x, name: str, n, lo: int, hi: int, dev) -> torch.Tensor:
    """at / prev of symbol_regime_panel: a 1-D integer array (numpy or torch, host or device) of n entries (n None:
    any length) with values in lo .. hi, as a contiguous int32 tensor on dev."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    want = "" if n is None else f" of shape {(n,)}"
    if x.dim() != 1 or x.dtype not in (torch.int32, torch.int64) or (n is not None and x.shape[0] != n):
        raise ValueError(f"{name}: expected a 1-D int32 / int64 tensor{want}")
    if x.numel() and (int(x.min()) < lo or int(x.max()) > hi):
        raise ValueError(f"{name}: values in {lo}..{hi} (context columns), got {int(x.min())}..{int(x.max())}")
    return x.to(device=dev, dtype=torch.int32).contiguous()


@device_entry
def symbol_regime_panel(feats: dict[str, torch.Tensor], close: torch.Tensor, *, rank: torch.Tensor | None = None,
                        at=None, prev=None, btc_return: torch.Tensor | None = None, btc_row: int | None = None,
                        seed=None, columns=REGIME_PANEL_COLUMNS) -> dict[str, torch.Tensor]:
    """The symbol_features entry every candle of a panel saw, for all symbols
    at once (bq_symbol_regime_panel): RegimeTransitionDetector.annotate_context
    (market_regime/regime_transitions.py:25-43, :162-232) over the feature
    columns of a context build. feats: the six FEATURE_COLUMNS [S, Tc] float64
    on one row stride, and close [S, Tc] they were computed from (a fresh
    build: CompactPanel.close, with rank = CompactPanel.rank, int32 [S, Tc]).
    at int [T_out]: the context column candle t sees (-1: none; default
    arange(Tc)); prev int [T_out]: the column stored before it (-1: none, -2:
    the seed; default at - 1). btc_return float64 [Tc]: BTC's return_pct per
    context column, NaN where it has no features (None: nowhere), btc_row its
    row (its own relative strength stays 0.0). seed: (int8 [S] micro-regime
    codes, negative None; float64 [S] strengths) of the snapshot before the
    panel's first context. Returns {name: [S, T_out]} for `columns`, a subset
    of REGIME_PANEL_COLUMNS: uint8 ok / micro_regime / micro_transition
    (indices into _lib.MICRO_REGIMES / MICRO_TRANSITIONS, _lib.MR_NONE for
    None) / above_ema20 / above_ema50, float64 rs_vs_btc /
    micro_regime_strength / micro_transition_strength / trend_score / atr_pct
    / bb_width (NaN where ok is 0). Columns left out are neither computed nor
    allocated."""
    columns = tuple(columns)
    _replay_columns("symbol_regime_panel", columns, REGIME_PANEL_COLUMNS)
    S, Tc = _replay_shape(close)
    missing = [n for n in FEATURE_COLUMNS if n not in feats]
    if missing:
        raise ValueError(f"feats: missing {missing} (expected {FEATURE_COLUMNS})")
    cols = [(feats[n], n) for n in FEATURE_COLUMNS] + [(close, "close")]
    _replay_panels(cols, S, Tc)
    for x, name in cols:
        if Tc > 1 and x.stride(1) != 1:
            raise ValueError(f"{name}: expected [S, T] with unit stride along T")
    ld_f = _row_stride(cols[0][0])
    if any(_row_stride(x) != ld_f for x, _ in cols[1:len(FEATURE_COLUMNS)]):
        raise ValueError("feature columns must share one row stride")
    if rank is not None and not (isinstance(rank, torch.Tensor) and rank.dtype == torch.int32
                                 and tuple(rank.shape) == (S, Tc) and (Tc <= 1 or rank.stride(1) == 1)):
        raise ValueError(f"rank: expected an int32 tensor of shape {(S, Tc)} with unit stride along T")
    dev = close.device
    if at is None:
        at_d = torch.arange(Tc, dtype=torch.int32, device=dev)
    else:
        at_d = _panel_index(at, "at", None, -1, Tc - 1, dev)
    T_out = int(at_d.shape[0])
    if prev is None:
        prev_d = (at_d - 1).clamp_(min=-1)
    else:
        prev_d = _panel_index(prev, "prev", T_out, -2, Tc - 1, dev)
    if btc_return is not None and not (isinstance(btc_return, torch.Tensor) and btc_return.dtype == torch.float64
                                       and tuple(btc_return.shape) == (Tc,)):
        raise ValueError(f"btc_return: expected a float64 tensor of shape {(Tc,)}")
    if btc_row is not None and not (isinstance(btc_row, int) and 0 <= btc_row < S):
        raise ValueError(f"btc_row: expected None or a row in 0..{S - 1}, got {btc_row}")
    if seed is not None and not (len(seed) == 2 and all(isinstance(x, torch.Tensor) for x in seed)
                                 and seed[0].dtype == torch.int8 and seed[1].dtype == torch.float64
                                 and all(tuple(x.shape) == (S,) and x.is_contiguous() for x in seed)):
        raise ValueError(f"seed: expected (micro_regime int8, micro_regime_strength float64) contiguous tensors of "
                         f"shape {(S,)}")
    sr, ss = seed if seed is not None else (None, None)
    _replay_on_device("symbol_regime_panel", [x for x, _ in cols] + [rank, btc_return, sr, ss])
    if btc_return is None:
        btc_return = torch.full((Tc,), float("nan"), dtype=torch.float64, device=dev)
    btc_return = btc_return.contiguous()
    out = {k: torch.empty((S, T_out), dtype=torch.uint8 if k in _lib.REGIME_PANEL_U8 else torch.float64, device=dev)
           for k in columns}
    st = _lib.load().bq_symbol_regime_panel(
        _lib.ptr_array([x.data_ptr() for x, _ in cols[:len(FEATURE_COLUMNS)]]), ld_f, _ptr(close),
        _row_stride(close), _ptr(rank), _row_stride(rank) if rank is not None else 0, S, Tc, _ptr(at_d), _ptr(prev_d),
        T_out, _ptr(btc_return), -1 if btc_row is None else btc_row, _ptr(sr), _ptr(ss),
        _lib.ptr_array([out[k].data_ptr() if k in out else 0 for k in _lib.REGIME_PANEL_U8]), T_out,
        _lib.ptr_array([out[k].data_ptr() if k in out else 0 for k in _lib.REGIME_PANEL_F64]), T_out,
        _stream_handle(None))
    _lib.check(st, "bq_symbol_regime_panel")
    return out


@device_entry
def context_partials(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    max_bars: int = 400,
    out: torch.Tensor | None = None,
    last: bool = False,
    stream: torch.cuda.Stream | None = None,
):
    """The [T, 10] breadth partials of every timestamp straight from the
    panel (bq_context_partials): market_features + breadth_partial fused, the
    feature columns never written (live_market_context_accumulator.py:95-163
    over _compute_symbol_features :244-297). Counts equal breadth_partial's,
    sums agree to rounding. last=True also returns the features at t = T - 1
    ({name: [S]}, what a context's symbol_features reads); returns
    (partial, last_features | None)."""
    hlc, S, T, ld_in = _hlc_panel(high, low, close)
    dev = hlc[2].device
    out = _partial_out(out, T, dev)
    lib = _lib.load()
    nbytes = int(lib.bq_context_workspace_bytes(S, T))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # caching allocator: 512-B aligned
    lastf = {n: torch.empty(S, dtype=torch.float64, device=dev) for n in FEATURE_COLUMNS} if last else None
    st = lib.bq_context_partials(
        _lib.ptr_array([t.data_ptr() for t in hlc]), S, T, ld_in, int(max_bars),
        ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(out.data_ptr()),
        _lib.ptr_array([lastf[n].data_ptr() for n in FEATURE_COLUMNS]) if last else None,
        _stream_handle(stream))
    _lib.check(st, "bq_context_partials")
    return out, lastf


class TickState:
    """Device-resident streaming state for S symbols (bq_state).

    ``frame`` is the per-message frame the reference re-enriches on every
    closed kline: KlinesProvider.LIMIT = 400 candles
    (consumers/klines_provider.py:40,201-215 -> producers/context_evaluator.py:
    367-371). Each tick returns the last row of indicators_enrichment over the
    symbol's last ``frame`` candles, the EMA family seeded at the frame's first
    candle exactly as the reference's re-enrichment is. ``frame=0`` keeps
    unbounded-history EMA carries (the full-series pandas EMA) instead."""

    FRAME = 400

    def __init__(self, n_symbols: int, params: IndicatorParams | None = None, frame: int = FRAME):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        p = (params or IndicatorParams()).to_c()
        # device memory of the state lives on the current device (bq_state_create)
        self.device = torch.device("cuda", torch.cuda.current_device())
        frame = int(frame)
        if frame != 0 and not (_lib.MAX_WINDOW + 2 <= frame <= 1 << 20):
            raise ValueError(f"frame must be 0 or in [{_lib.MAX_WINDOW + 2}, {1 << 20}], got {frame}")
        _lib.check(self._lib.bq_state_create_frame(ctypes.byref(self._h), int(n_symbols), ctypes.byref(p), frame),
                   "bq_state_create_frame")
        self.n_symbols = int(n_symbols)
        self.frame = frame

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.bq_state_destroy(h)
            self._h = None

    @property
    def count(self) -> int:
        return int(self._lib.bq_state_count(self._h))

    @device_entry
    def seed(self, open_, high, low, close, volume, stream=None) -> None:
        close = _check_panel(close, "close")
        S, T = close.shape
        if S != self.n_symbols:
            raise ValueError(f"seed panel has {S} symbols, state has {self.n_symbols}")
        if close.device != self.device:
            raise ValueError(f"seed panel on {close.device}, state on {self.device}")
        ins = _panels((open_, high, low, close, volume), INPUT_FIELDS, S, T)
        st = self._lib.bq_state_seed(
            self._h, _lib.ptr_array([t.data_ptr() for t in ins]), T, T, _stream_handle(stream)
        )
        _lib.check(st, "bq_state_seed")

    @device_entry
    def tick(self, new_ohlcv, out: dict[str, torch.Tensor] | None = None, columns=ENRICH_COLUMNS, stream=None):
        """new_ohlcv: sequence of 5 float64 CUDA vectors [S] (open, high, low, close, volume)."""
        vecs = []
        for t, n in zip(new_ohlcv, INPUT_FIELDS):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.numel() == self.n_symbols):
                raise ValueError(f"{n}: expected float64 CUDA vector of length {self.n_symbols}")
            if t.device != self.device:
                raise ValueError(f"{n}: on {t.device}, state on {self.device}")
            vecs.append(t.contiguous())
        out = dict(out or {})
        cols = tuple(columns)
        dev = vecs[0].device
        for n in cols:
            if n not in out:
                out[n] = torch.empty(self.n_symbols, dtype=torch.float64, device=dev)
            else:
                o = out[n]
                if not (isinstance(o, torch.Tensor) and o.dtype == torch.float64 and o.device == dev
                        and o.numel() == self.n_symbols and o.is_contiguous()):
                    raise ValueError(f"out[{n}]: expected a contiguous float64 vector of {self.n_symbols} on {dev}")
        st = self._lib.bq_tick(
            self._h,
            _lib.ptr_array([t.data_ptr() for t in vecs]),
            _lib.ptr_array([out[n].data_ptr() if n in cols else 0 for n in ENRICH_COLUMNS]),
            _stream_handle(stream),
        )
        _lib.check(st, "bq_tick")
        return {n: out[n] for n in cols}


@device_entry
def beta_corr(
    close: torch.Tensor,
    btc_close: torch.Tensor,
    window: int = 50,
    stream: torch.cuda.Stream | None = None,
) -> dict[str, torch.Tensor]:
    """Rolling beta / correlation of log returns vs the benchmark at every t
    (ContextEvaluator.dynamic_btc_beta_corr, producers/context_evaluator.py:154-194).
    close: [S, T]; btc_close: [T] index-aligned with the panel.

    Missing (NaN) and zero closes follow the reference's dropna on every
    prefix [0, t]: the window at t is the last `window` valid return pairs,
    however far back they lie; NaN while fewer exist, while the benchmark's
    variance is 0, and while the window holds a +-inf return (a zero close).
    A candle without a pair of its own (either close missing at t or t - 1)
    returns the last valid pair's value, so [:, -1] is the reference's
    iloc[-1] (oracle.indicators_ref.beta_corr_prefix)."""
    close = _check_panel(close, "close")
    S, T = close.shape
    btc = _check_panel(btc_close.reshape(1, -1), "btc_close", (1, T)).contiguous()
    beta = torch.empty((S, T), dtype=torch.float64, device=close.device)
    corr = torch.empty_like(beta)
    # the benchmark's log returns (log(c / c.shift(1)), :166-169) and window
    # stats once per call, in the kernel's one-workgroup pre-pass (scratch)
    scratch = torch.empty(4 * T, dtype=torch.float64, device=close.device)
    st = _lib.load().bq_beta_corr_ws(
        ctypes.c_void_p(close.data_ptr()), ctypes.c_void_p(btc.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
        S, T, _row_stride(close),
        int(window), ctypes.c_void_p(beta.data_ptr()), ctypes.c_void_p(corr.data_ptr()), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_beta_corr_ws")
    return {"beta": beta, "corr": corr}


def _signal_launch(name: str, ins: list[torch.Tensor], window: int, stream) -> torch.Tensor:
    S, T = ins[-1].shape
    ld = _row_stride(ins[0])
    if any(_row_stride(t) != ld for t in ins):
        ins = [t.contiguous() for t in ins]
        ld = T
    out = torch.empty((S, T), dtype=torch.float64, device=ins[0].device)
    st = getattr(_lib.load(), name)(*[ctypes.c_void_p(t.data_ptr()) for t in ins], S, T, ld, int(window),
                                    ctypes.c_void_p(out.data_ptr()), T, _stream_handle(stream))
    _lib.check(st, name)
    return out


@device_entry
def wilder_rsi(close: torch.Tensor, window: int = 14, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """MeanReversionFade._rsi (strategies/mean_reversion_fade.py:88-109) at
    every t, time-parallel (bq_wilder_rsi; 1e-9 of pandas, finite closes)."""
    close = _check_panel(close, "close")
    return _signal_launch("bq_wilder_rsi", [close], window, stream)


@device_entry
def zscore(close: torch.Tensor, window: int = 20, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """RangeBbRsiMeanReversion._compute_zscore (strategies/range_bb_rsi_mean_reversion.py:132-138)
    at every t, time-parallel (bq_zscore)."""
    close = _check_panel(close, "close")
    return _signal_launch("bq_zscore", [close], window, stream)


@device_entry
def adx(high: torch.Tensor, low: torch.Tensor, close: torch.Tensor, window: int = 14,
        stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """RangeBbRsiMeanReversion._compute_adx (strategies/range_bb_rsi_mean_reversion.py:101-130)
    at every t, time-parallel (bq_adx, window <= 64)."""
    close = _check_panel(close, "close")
    S, T = close.shape
    return _signal_launch("bq_adx", [_check_panel(high, "high", (S, T)), _check_panel(low, "low", (S, T)), close],
                          window, stream)


@device_entry
def rolling(
    x: torch.Tensor,
    window: int,
    stat: str = "mean",
    q: float = 0.5,
    min_periods: int | None = None,
    shift: int = 0,
    out: torch.Tensor | None = None,
    stream: torch.cuda.Stream | None = None,
) -> torch.Tensor:
    """x.shift(shift).rolling(window, min_periods).<stat>() along T of a [S, T]
    panel; stat in {"quantile", "median", "mean", "sum", "var", "std", "max",
    "min", "isum"} (var / std: ddof 1; isum: the sum of an integer-valued
    series such as a flag count — pandas' value, computed without the
    sequential replay)."""
    x = _check_panel(x, "x")
    S, T = x.shape
    if stat == "max":
        stat, q = "quantile", 1.0
    elif stat == "min":
        stat, q = "quantile", 0.0
    if stat not in _lib.ROLL_MODES:
        raise ValueError(f"unknown rolling statistic {stat!r}")
    if out is None:
        out = torch.empty((S, T), dtype=torch.float64, device=x.device)
    st = _lib.load().bq_rolling(
        ctypes.c_void_p(x.data_ptr()), S, T, _row_stride(x), int(window),
        int(window if min_periods is None else min_periods), int(shift), _lib.ROLL_MODES[stat], float(q),
        ctypes.c_void_p(out.data_ptr()), _row_stride(out), _stream_handle(stream),
    )
    _lib.check(st, "bq_rolling")
    return out


@device_entry
def rolling_quantile_cross(
    x: torch.Tensor,
    window: int,
    q: float,
    min_periods: int | None = None,
    shift: int = 0,
    stream: torch.cuda.Stream | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """(thr, cross): thr = x.shift(shift).rolling(window, min_periods).quantile(q)
    and cross = (x >= thr) & (x.shift(1) < thr.shift(1)) (bool) in one pass
    where the sliding-window kernel runs (bq_rolling_quantile_cross) —
    LiquidationSweepPump's score_threshold / score_cross
    (strategies/liquidation_sweep_pump.py:231-239)."""
    x = _check_panel(x, "x")
    S, T = x.shape
    thr = torch.empty((S, T), dtype=torch.float64, device=x.device)
    cross = torch.empty((S, T), dtype=torch.bool, device=x.device)
    st = _lib.load().bq_rolling_quantile_cross(
        ctypes.c_void_p(x.data_ptr()), S, T, _row_stride(x), int(window),
        int(window if min_periods is None else min_periods), int(shift), float(q),
        ctypes.c_void_p(thr.data_ptr()), T, ctypes.c_void_p(cross.data_ptr()), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_rolling_quantile_cross")
    return thr, cross


@device_entry
def ewm(
    x: torch.Tensor,
    alpha: float | None = None,
    span: float | None = None,
    min_periods: int = 0,
    out: torch.Tensor | None = None,
    stream: torch.cuda.Stream | None = None,
) -> torch.Tensor:
    """x.ewm(alpha|span, adjust=False, min_periods).mean() along T (pandas'
    exact recursion, NaN gaps decay the old weight)."""
    x = _check_panel(x, "x")
    S, T = x.shape
    if (alpha is None) == (span is None):
        raise ValueError("give exactly one of alpha / span")
    # pandas: comass from span or alpha, alpha = 1 / (1 + comass)
    com = (float(span) - 1.0) / 2.0 if span is not None else 1.0 / float(alpha) - 1.0
    a = 1.0 / (1.0 + com)
    if out is None:
        out = torch.empty((S, T), dtype=torch.float64, device=x.device)
    st = _lib.load().bq_ewm(
        ctypes.c_void_p(x.data_ptr()), S, T, _row_stride(x), a, int(min_periods),
        ctypes.c_void_p(out.data_ptr()), _row_stride(out), _stream_handle(stream),
    )
    _lib.check(st, "bq_ewm")
    return out


@dataclass
class Roll:
    """One x.shift(shift).rolling(window, min_periods).<stat>() series of a
    rolling_many batch (stat as in rolling())."""

    x: torch.Tensor
    window: int
    stat: str = "mean"
    q: float = 0.5
    min_periods: int | None = None
    shift: int = 0


@dataclass
class Ewm:
    """One x.ewm(alpha|span, adjust=False, min_periods).mean() series of a batch."""

    x: torch.Tensor
    alpha: float | None = None
    span: float | None = None
    min_periods: int = 0


@dataclass
class Ffill:
    """x.ffill() along T (leading NaNs stay) as one series of a batch."""

    x: torch.Tensor


@device_entry
def rolling_many(*specs, exact: bool = True, stream: torch.cuda.Stream | None = None,
                 cross: tuple[int, ...] = ()):
    """Independent Roll / Ewm / Ffill series over one [S, T] shape in as few
    launches as the kernel families allow (bq_rolling_batch): the
    lane-per-symbol replays of different series run side by side instead of
    one launch each. A moment / ewm / ffill series may have fewer rows than
    the panel (e.g. the [1, T] benchmark beside an [S, T] panel): it joins
    the same launch (bq_roll_job.rows) instead of paying a replay walk of
    its own. exact=False: sums / means (window + shift <= 128) and ewm run
    time-parallel (bq_panel.hip, panel mode), within rounding of pandas
    (1e-9) instead of the bit-exact sequential replay; order statistics on
    the tile kernels sort packed keys (the union slot in the key's low bits:
    the selected value is an element within 2^-45 relative of the exact
    order statistic); var / std and the rest are unchanged.
    cross: indices of quantile specs that also get their crossing flags,
    (x >= thr) & (x.shift(1) < thr.shift(1)) as bool [S, T]
    (bq_rolling_batch_cross; liquidation_sweep_pump.py:237-239's score_cross
    form) — then the result is (outs, flags), flags in the order of cross."""
    if not specs:
        return ([], []) if cross else []
    xs = [_check_panel(sp.x, "x") for sp in specs]
    S = max(int(x.shape[0]) for x in xs)
    T = int(xs[0].shape[1])
    outs: list[torch.Tensor] = []
    jobs = []
    keep = []
    for sp, x in zip(specs, xs):
        rows = int(x.shape[0])
        if x.shape[1] != T:
            raise ValueError(f"x: shape {tuple(x.shape)}: every series of a batch needs T = {T}")
        if rows != S and isinstance(sp, Roll) and sp.stat not in ("mean", "sum", "var", "std", "var0", "std0"):
            raise ValueError(f"x: shape {tuple(x.shape)} != {(S, T)} (only moments, ewm and ffill may have fewer rows)")
        out = torch.empty((rows, T), dtype=torch.float64, device=x.device)
        j = _lib.BqRollJob()
        j.x, j.out, j.ld_in, j.ld_out = x.data_ptr(), out.data_ptr(), _row_stride(x), T
        j.rows = rows if rows != S else 0
        j.panel = 0 if exact else 1
        if isinstance(sp, Ffill):
            j.mode = _lib.ROLL_FFILL
        elif isinstance(sp, Ewm):
            if (sp.alpha is None) == (sp.span is None):
                raise ValueError("give exactly one of alpha / span")
            com = (float(sp.span) - 1.0) / 2.0 if sp.span is not None else 1.0 / float(sp.alpha) - 1.0
            j.alpha, j.mode, j.min_periods = 1.0 / (1.0 + com), _lib.ROLL_EWM, int(sp.min_periods)
        else:
            stat, q = sp.stat, sp.q
            if stat == "max":
                stat, q = "quantile", 1.0
            elif stat == "min":
                stat, q = "quantile", 0.0
            if stat not in _lib.ROLL_MODES:
                raise ValueError(f"unknown rolling statistic {stat!r}")
            j.window, j.shift, j.mode, j.q = int(sp.window), int(sp.shift), _lib.ROLL_MODES[stat], float(q)
            j.min_periods = int(sp.window if sp.min_periods is None else sp.min_periods)
        jobs.append(j)
        outs.append(out)
        keep.append(x)
    flags = {}
    for k in cross:
        if not (isinstance(specs[k], Roll) and specs[k].stat == "quantile" and xs[k].shape[0] == S):
            raise ValueError(f"cross: spec {k} is not a quantile over the whole panel")
        flags[k] = torch.empty((S, T), dtype=torch.bool, device=xs[k].device)
    fptr = {id(jobs[k]): flags[k].data_ptr() for k in flags}
    L = _lib.load()
    # a batch call takes MAX_ROLL_JOBS jobs: the sequential replays (moments,
    # ewm — one latency-bound launch per call, whatever its job count) go
    # into the calls first, so 14 replays + 4 order statistics make one replay
    # launch instead of a second one for the replays that spilled into the
    # next call (outputs stay in spec order: each job carries its own pointer)
    _REPLAY = (_lib.ROLL_EWM,) + tuple(_lib.ROLL_MODES[k] for k in ("mean", "sum", "var", "std", "var0", "std0"))
    jobs = sorted(jobs, key=lambda j: 0 if j.mode in _REPLAY else 1)
    for i in range(0, len(jobs), _lib.MAX_ROLL_JOBS):
        chunk = jobs[i : i + _lib.MAX_ROLL_JOBS]
        arr = (_lib.BqRollJob * len(chunk))(*chunk)
        if fptr:
            cp = _lib.ptr_array([fptr.get(id(j), 0) for j in chunk])
            cl = (ctypes.c_int64 * len(chunk))(*([T] * len(chunk)))
            _lib.check(L.bq_rolling_batch_cross(arr, len(chunk), S, T, cp, cl, _stream_handle(stream)),
                       "bq_rolling_batch_cross")
        else:
            _lib.check(L.bq_rolling_batch(arr, len(chunk), S, T, _stream_handle(stream)), "bq_rolling_batch")
    return (outs, [flags[k] for k in cross]) if cross else outs


@device_entry
def row_quantile(x: torch.Tensor, q: float, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """numpy.quantile(row[~isnan(row)], q) per row (numpy 'linear' method), as
    FailedSpikeFade.auto_calibrate (strategies/failed_spike_fade.py:229-257)
    calls it. Returns [S] float64, NaN for rows without observations."""
    x = _check_panel(x, "x")
    S, T = x.shape
    out = torch.empty((S,), dtype=torch.float64, device=x.device)
    st = _lib.load().bq_row_quantile(
        ctypes.c_void_p(x.data_ptr()), S, T, _row_stride(x), float(q), ctypes.c_void_p(out.data_ptr()),
        _stream_handle(stream),
    )
    _lib.check(st, "bq_row_quantile")
    return out


@device_entry
def cooldown(label: torch.Tensor, bars: int, stream: torch.cuda.Stream | None = None):
    """FailedSpikeFade.apply_cooldown (strategies/failed_spike_fade.py:495-520):
    returns (kept, suppressed) bool [S, T] — a label within `bars` candles of
    the last kept label is cleared and flagged suppressed."""
    if not isinstance(label, torch.Tensor) or not label.is_cuda or label.dtype != torch.bool:
        raise ValueError("label: expected a bool CUDA tensor (no CPU path)")
    if label.dim() == 1:
        label = label.unsqueeze(0)
    label = label.contiguous()
    S, T = label.shape
    kept = torch.empty_like(label)
    sup = torch.empty_like(label)
    st = _lib.load().bq_cooldown(
        ctypes.c_void_p(label.data_ptr()), S, T, T, int(bars), ctypes.c_void_p(kept.data_ptr()),
        ctypes.c_void_p(sup.data_ptr()), T, _stream_handle(stream),
    )
    _lib.check(st, "bq_cooldown")
    return kept, sup


@device_entry
def supertrend(
    high: torch.Tensor,
    low: torch.Tensor,
    close: torch.Tensor,
    period: int = 10,
    multiplier: float = 3.0,
    atr: torch.Tensor | None = None,
    stream: torch.cuda.Stream | None = None,
    exact: bool = True,
) -> dict[str, torch.Tensor]:
    """pybinbot Indicators.set_supertrend (strategies/coinrule/coinrule.py:143-160)
    on a [S, T] panel: {"supertrend": bool (uptrend), "supertrend_upper",
    "supertrend_lower": final bands}. ATR = TR.rolling(period).mean() unless
    given: the default exact=True forms it in the same walk as pandas'
    roll_mean (bq_supertrend_hlc, bit for bit — the live path,
    Indicators.set_supertrend); exact=False is the panel mode
    (bq_supertrend_panel: chunks of each row walked in parallel with verified
    chunk starts, the same recursion) on an ATR equal to pandas' to rounding,
    so bands agree to rounding and flags up to near-ties."""
    high = _check_panel(high, "high")
    S, T = high.shape
    low = _check_panel(low, "low", (S, T))
    close = _check_panel(close, "close", (S, T))
    up = torch.empty((S, T), dtype=torch.bool, device=close.device)
    upper = torch.empty((S, T), dtype=torch.float64, device=close.device)
    lower = torch.empty_like(upper)
    if atr is None:
        ins = [t.contiguous() for t in (high, low, close)]
        L = _lib.load()
        args = [_lib.ptr_array([t.data_ptr() for t in ins]), S, T, T, int(period), float(multiplier),
                ctypes.c_void_p(up.data_ptr()), ctypes.c_void_p(upper.data_ptr()), ctypes.c_void_p(lower.data_ptr()),
                T]
        if exact:
            fn = "bq_supertrend_hlc"
            st = L.bq_supertrend_hlc(*args, _stream_handle(stream))
        else:
            fn = "bq_supertrend_panel"
            st = L.bq_supertrend_panel(*args, _stream_handle(stream))
        _lib.check(st, fn)
    else:
        atr = _check_panel(atr, "atr", (S, T))
        ins = [t.contiguous() for t in (high, low, close, atr)]
        st = _lib.load().bq_supertrend(
            _lib.ptr_array([t.data_ptr() for t in ins]), S, T, T, float(multiplier), ctypes.c_void_p(up.data_ptr()),
            ctypes.c_void_p(upper.data_ptr()), ctypes.c_void_p(lower.data_ptr()), T, _stream_handle(stream),
        )
        _lib.check(st, "bq_supertrend")
    return {"supertrend": up, "supertrend_upper": upper, "supertrend_lower": lower}


# ---- frame plumbing: resample / timestamp joins (bq_frame.hip) -----------------


def _check_ts(ts: torch.Tensor, name: str = "ts") -> torch.Tensor:
    if not isinstance(ts, torch.Tensor) or not ts.is_cuda or ts.dtype != torch.int64:
        raise ValueError(f"{name}: expected an int64 CUDA tensor of ms timestamps (no CPU path)")
    if ts.dim() == 1:
        ts = ts.unsqueeze(0)
    return ts.contiguous()


def _check_lens(lens, S: int, device) -> torch.Tensor | None:
    if lens is None:
        return None
    if not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(lens, dtype=torch.int64)
    lens = lens.to(device=device, dtype=torch.int64).contiguous()
    if lens.numel() != S:
        raise ValueError(f"lens: expected {S} entries, got {lens.numel()}")
    return lens


def _ptr(t: torch.Tensor | None) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


@device_entry
def resample(
    ts: torch.Tensor,
    fields: dict[str, torch.Tensor],
    aggs: dict[str, str],
    interval_ms: int,
    lens=None,
    max_bins: int | None = None,
    tail: bool = False,
    stream: torch.cuda.Stream | None = None,
) -> tuple[torch.Tensor, dict[str, torch.Tensor], torch.Tensor]:
    """Candles.resample (producers/context_evaluator.py:403-407) on a ragged
    [S, T] panel: pandas resample(interval, origin="start_day").agg(aggs) on
    the open_time index. Returns (bin labels int64 [S, B], {field: [S, B]},
    bins per row int64 [S]); B = the longest row's bin count, read back from
    the device — or, with max_bins (fixed frame geometry, e.g. a captured
    graph: no host synchronisation), B = max_bins, which must be at least
    every row's bin count (bins past a row's count are left unwritten) —
    or, with tail=True (bq_resample_tail), a row with more bins than B keeps
    its newest B bins, so bin min(bins, B) - 1 is always the row's latest
    (the returned bins per row stay the true counts)."""
    ts = _check_ts(ts)
    S, T = ts.shape
    names = list(fields)
    if len(names) > _lib.MAX_RESAMPLE_FIELDS:
        raise ValueError(f"at most {_lib.MAX_RESAMPLE_FIELDS} fields per resample call")
    ins = [_check_panel(fields[n], n, (S, T)).contiguous() for n in names]
    codes = []
    for n in names:
        a = aggs.get(n)
        if a not in _lib.AGG_CODES:
            raise ValueError(f"{n}: aggregation {a!r} not in {sorted(_lib.AGG_CODES)}")
        codes.append(_lib.AGG_CODES[a])
    lens = _check_lens(lens, S, ts.device)
    L = _lib.load()
    out_lens = torch.empty(S, dtype=torch.int64, device=ts.device)
    _lib.check(L.bq_resample_count(_ptr(ts), _ptr(lens), S, T, T, int(interval_ms), _ptr(out_lens),
                                   _stream_handle(stream)), "bq_resample_count")
    if max_bins is not None:
        if max_bins < 0:
            raise ValueError("max_bins must be >= 0")
        B = int(max_bins)
    else:
        B = int(out_lens.max().item()) if S else 0
    out_ts = torch.empty((S, B), dtype=torch.int64, device=ts.device)
    outs = [torch.empty((S, B), dtype=torch.float64, device=ts.device) for _ in names]
    agg_arr = (ctypes.c_int32 * max(1, len(codes)))(*codes)
    st = (L.bq_resample_tail if tail else L.bq_resample)(
        _ptr(ts), _lib.ptr_array([t.data_ptr() for t in ins]), ctypes.cast(agg_arr, ctypes.c_void_p), len(names),
        _ptr(lens), S, T, T, int(interval_ms), _ptr(out_ts), _lib.ptr_array([t.data_ptr() for t in outs]), B,
        _stream_handle(stream),
    )
    _lib.check(st, "bq_resample")
    return out_ts, dict(zip(names, outs)), out_lens


@device_entry
def align(ts: torch.Tensor, bench_ts: torch.Tensor, bench_val: torch.Tensor, lens=None,
          stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Benchmark value at each candle's timestamp (left merge on open_time,
    duplicates keep "last"; strategies/liquidation_sweep_pump.py:255-263),
    NaN where the benchmark has no candle. ts [S, T] int64, bench_ts [Tb]
    ascending, bench_val [Tb] float64."""
    ts = _check_ts(ts)
    S, T = ts.shape
    bts = _check_ts(bench_ts, "bench_ts").reshape(-1)
    bval = _check_panel(bench_val.reshape(1, -1), "bench_val", (1, bts.numel())).contiguous()
    lens = _check_lens(lens, S, ts.device)
    out = torch.empty((S, T), dtype=torch.float64, device=ts.device)
    st = _lib.load().bq_align(_ptr(ts), _ptr(lens), S, T, T, _ptr(bts), _ptr(bval), bts.numel(), _ptr(out), T,
                              _stream_handle(stream))
    _lib.check(st, "bq_align")
    return out


LEADERSHIP_FUSED = dict(lookback=96, long_max=31)   # bq_leadership's compiled configuration


@device_entry
def leadership(open_time: torch.Tensor, close: torch.Tensor, bench_ts: torch.Tensor, bench_close: torch.Tensor,
               rs_quantile: float = 0.80, lookback: int = 96, min_history: int = 100, min_count: int = 20,
               short: int = 8, long: int = 24, stream: torch.cuda.Stream | None = None):
    """GradualGainerRetest._leadership_allows at every prefix t
    (strategies/gradual_gainer_retest.py:131-196) in one pass (bq_leadership:
    the thresholds are never formed — "rs >= sorted(h)[a]" is a count of the
    window's entries <= rs): returns {"leader": bool [S, T], "rs_2h": [S, T],
    "rs_6h": [S, T]}, or None when the parameters are not the compiled ones
    (RS_LOOKBACK 96, long <= 31): the caller then runs the staged pipeline."""
    if lookback != LEADERSHIP_FUSED["lookback"] or not 0.0 <= rs_quantile < 1.0 \
            or not 1 <= short <= long <= LEADERSHIP_FUSED["long_max"] or min_count < 1 or min_history < 0:
        return None
    close = _check_panel(close, "close").contiguous()
    S, T = close.shape
    ts = _check_ts(open_time)
    if tuple(ts.shape) != (S, T):
        raise ValueError(f"open_time: expected shape {(S, T)}, got {tuple(ts.shape)}")
    bts = _check_ts(bench_ts, "bench_ts").reshape(-1).contiguous()
    bc = _check_panel(bench_close.reshape(1, -1), "bench_close", (1, bts.numel())).contiguous()
    dev = close.device
    leader = torch.empty((S, T), dtype=torch.bool, device=dev)
    rs2 = torch.empty((S, T), dtype=torch.float64, device=dev)
    rs6 = torch.empty_like(rs2)
    lib = _lib.load()
    nbytes = int(lib.bq_leadership_workspace_bytes(S, T))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # caching allocator: 512-B aligned
    st = lib.bq_leadership(_ptr(ts), T, _ptr(close), T, S, T, _ptr(bts), _ptr(bc), bts.numel(), float(rs_quantile),
                           int(lookback), int(min_history), int(min_count), int(short), int(long), _ptr(ws), nbytes,
                           _ptr(leader), _ptr(rs2), _ptr(rs6), T, _stream_handle(stream))
    _lib.check(st, "bq_leadership")
    return {"leader": leader, "rs_2h": rs2, "rs_6h": rs6}


IMPULSE_TILE = _lib.IMPULSE_TILE   # candles per workgroup tile of bq_impulse_rider / bq_bb_stable
IMPULSE_DEFAULTS = dict(   # RelativeStrengthImpulseRider's class attributes (:36-46)
    min_history=20, min_impulse=0.05, max_impulse=0.18, min_rs=0.08, max_btc_return=0.01, min_conf_return=0.0,
    min_close_location=0.70, max_atr_pct=0.06, entry_factor=1 - 1.0 / 100)


def _gate_rows(v, name: str, S: int):
    """lens / first_t: None or S integers (checked before any device work)."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError(f"{name}: expected an integer tensor, got {v.dtype}")
        if v.numel() != S:
            raise ValueError(f"{name}: expected {S} entries, got {v.numel()}")
        return v
    v = torch.as_tensor(v, dtype=torch.int64)
    if v.numel() != S:
        raise ValueError(f"{name}: expected {S} entries, got {v.numel()}")
    return v


def _common_pitch(cols: list[torch.Tensor]) -> tuple[list[torch.Tensor], int]:
    """The columns on one row pitch (as given when they share one — e.g. the
    padded enrich views — else contiguous copies)."""
    ld = _row_stride(cols[0])
    if any(_row_stride(c) != ld for c in cols[1:]):
        cols = [c.contiguous() for c in cols]
        ld = _row_stride(cols[0])
    return cols, ld


# ---- the argument layer of the strategy entry points on a [S, T] panel: the tile-mapped entries (impulse_rider,
# bb_stable, top_gainer_entry, sweep_select), spike_frames and the nine replay wrappers (retest, spike_fade,
# price_tracker, mean_reversion, range_fade, buy_the_dip, bb_extreme, rs_reversal, grid_ladder). Each check raises the
# text the wrappers raised themselves, with the entry's name substituted

def _replay_params(entry: str, defaults: dict, params: dict, int_keys=None, noun: str = "parameters") -> dict:
    """defaults overlaid with params; int_keys given: every other parameter is a finite float."""
    bad = set(params) - set(defaults)
    if bad:
        raise ValueError(f"{entry}: unknown {noun} {sorted(bad)} (known: {sorted(defaults)})")
    par = {**defaults, **params}
    if int_keys is not None:
        for k, val in par.items():
            if k not in int_keys and not math.isfinite(float(val)):
                raise ValueError(f"{entry}: {k} must be finite, got {val}")
    return par


def _replay_struct(cls, par: dict, int_keys):
    p = cls()
    for k, val in par.items():
        setattr(p, k, int(val) if k in int_keys else float(val))
    return p


def _replay_columns(entry: str, columns, known, tail: bool = True) -> None:
    unknown = [k for k in columns if k not in known]
    if unknown:
        raise ValueError(f"{entry}: unknown columns {unknown}" + (f" (known: {known})" if tail else ""))


def _replay_shape(c, name: str = "close") -> tuple[int, int]:
    if not isinstance(c, torch.Tensor) or c.dim() != 2:
        raise ValueError(f"{name}: expected [S, T] with unit stride along T")
    return c.shape


def _replay_panels(pairs, S: int, T: int) -> None:
    """(tensor, name) pairs: float64 [S, T]."""
    for x, name in pairs:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64:
            raise ValueError(f"{name}: expected dtype float64, got {getattr(x, 'dtype', type(x))}")
        if tuple(x.shape) != (S, T):
            raise ValueError(f"{name}: shape {tuple(x.shape)} != {(S, T)}")


_BOOL = (torch.bool,)


def _replay_flags(pairs, S: int, T: int, dtypes=_BOOL, dev: bool = False, pitch: bool = False):
    """(tensor, name) pairs: flag panels [S, T] of one of dtypes. dev False:
    that check alone, on the host. dev True: each is on the device as well,
    and they are returned with unit stride along T (a flag of another stride
    is copied), each on its own row pitch; pitch: on one common row pitch,
    as (flags, pitch)."""
    for x, name in pairs:
        if not isinstance(x, torch.Tensor) or x.dtype not in dtypes or tuple(x.shape) != (S, T):
            raise ValueError(f"{name}: expected a bool tensor of shape {(S, T)}")
        if dev and not x.is_cuda:
            raise ValueError(f"{name}: expected a CUDA tensor (no CPU path)")
    if not dev:
        return None
    flags = [x if T <= 1 or x.stride(1) == 1 else x.contiguous() for x, _ in pairs]
    return _common_pitch(flags) if pitch else flags


def _replay_features(features, names) -> list:
    """features: None (formed in the pass) or one tensor per name; as (tensor, name) pairs."""
    if features is None:
        return []
    if len(features) != len(names):
        raise ValueError(f"features: expected {names}")
    return list(zip(features, names))


def _replay_time(x, name: str, S: int, T: int) -> None:
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or tuple(x.shape) != (S, T):
        raise ValueError(f"{name}: expected an int64 tensor of shape {(S, T)}")


def _replay_ctx(ctx, ctx_ok, rows, T: int):
    """ctx float64 [len(rows), Tc], Tc 1 or T, and ctx_ok [Tc] or None. Returns
    (ctx, ctx_ok, Tc, ld_ctx) with unit stride along Tc."""
    n = len(rows)
    if (not isinstance(ctx, torch.Tensor) or ctx.dtype != torch.float64 or ctx.dim() != 2
            or ctx.shape[0] != n or ctx.shape[1] not in (1, T)):
        raise ValueError(f"ctx: expected a float64 tensor of shape {(n, 1)} or {(n, T)} (rows {rows})")
    Tc = int(ctx.shape[1])
    if ctx_ok is not None and (not isinstance(ctx_ok, torch.Tensor) or ctx_ok.dtype not in (torch.bool, torch.uint8)
                               or tuple(ctx_ok.shape) != (Tc,)):
        raise ValueError(f"ctx_ok: expected a bool / uint8 tensor of shape {(Tc,)}")
    if (Tc > 1 and ctx.stride(1) != 1) or ctx.stride(0) < Tc:
        ctx = ctx.contiguous()
    if ctx_ok is not None and not ctx_ok.is_contiguous():
        ctx_ok = ctx_ok.contiguous()
    return ctx, ctx_ok, Tc, int(ctx.stride(0))


def _replay_sym(sym, spec, S: int, T: int):
    """sym: None or one tensor per (name, dtypes) of spec, all [S] or all [S, T].
    Returns (the tensors, contiguous, or a None per entry; ld_sym: T or 0)."""
    if sym is None:
        return [None] * len(spec), 0
    if len(sym) != len(spec):
        raise ValueError(f"sym: expected {tuple(n for n, _ in spec)}")
    shp = tuple(getattr(sym[0], "shape", ()))
    if shp not in ((S,), (S, T)):
        raise ValueError(f"sym: expected tensors of shape {(S,)} or {(S, T)}")
    for x, (name, dts) in zip(sym, spec):
        if not isinstance(x, torch.Tensor) or x.dtype not in dts or tuple(x.shape) != shp:
            raise ValueError(f"sym.{name}: expected a {dts[0]} tensor of shape {shp}")
    return [x.contiguous() for x in sym], (T if len(shp) == 2 else 0)


def _replay_state(state, names, dtypes, S: int):
    """state: None or one contiguous [S] tensor per name. Returns them, or a None per name."""
    if state is None:
        return (None,) * len(names)
    if len(state) != len(names):
        raise ValueError(f"state: expected ({', '.join(names)})")
    for x, name, dt in zip(state, names, dtypes):
        if not isinstance(x, torch.Tensor) or x.dtype != dt or tuple(x.shape) != (S,) or not x.is_contiguous():
            raise ValueError(f"state.{name}: expected a contiguous {dt} tensor of shape {(S,)}")
    return tuple(state)


def _replay_rows(lens, first_t, from_t, S: int, dev=None):
    """lens / first_t / from_t (None throughout for an entry without it): gated
    on the host (dev None), or as int64 [S] on dev."""
    rows = zip((lens, first_t, from_t), ("lens", "first_t", "from_t"))
    if dev is None:
        return tuple(_gate_rows(v, name, S) for v, name in rows)
    return tuple(_check_lens(v, S, dev) for v, _ in rows)


def _replay_on_device(label: str, tensors) -> None:
    if not all(x.is_cuda for x in tensors if x is not None):
        raise ValueError(f"{label}: expected CUDA tensors (no CPU path)")


def _replay_outputs(columns, known, S: int, T: int, dev):
    """status uint8 [S, T], {name: float64 [S, T]} for columns, and the values' pointer array in `known` order."""
    status = torch.empty((S, T), dtype=torch.uint8, device=dev)
    outs = {k: torch.empty((S, T), dtype=torch.float64, device=dev) for k in columns}
    return status, outs, _lib.ptr_array([outs[k].data_ptr() if k in outs else 0 for k in known])


@device_entry
def impulse_rider(o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, atr: torch.Tensor,
                  open_time: torch.Tensor, bench_ts: torch.Tensor, bench_close: torch.Tensor, *, first_t=None,
                  lens=None, columns=_lib.IMPULSE_VALUES, check_bench: bool = True, **thresholds):
    """RelativeStrengthImpulseRider._features at every prefix t
    (strategies/relative_strength_impulse_rider.py:92-198; bq_impulse_rider):
    column t of row s = the method on df.iloc[first_t[s]:t + 1] against the
    benchmark frame (bench_ts ascending, a repeated time resolves to its last
    row). Panels [S, T] float64 with unit stride along T and any row pitch,
    open_time [S, T] int64 ms. Returns (values, status): values maps each name
    of `columns` (a subset of _lib.IMPULSE_VALUES; others are not computed)
    to [S, T] float64 — the method's value where status == 0, NaN elsewhere —
    and status is [S, T] uint8 (_lib.BQ_IR_*; BQ_IR_NO_FRAME where
    t >= lens[s]). thresholds: IMPULSE_DEFAULTS' keys. check_bench: verify
    that bench_ts ascends (ValueError otherwise; one small reduction read
    back to the host, skipped while a graph is being captured) — False for
    callers that built the benchmark frame themselves."""
    par = _replay_params("impulse_rider", IMPULSE_DEFAULTS, thresholds, noun="thresholds")
    if int(par["min_history"]) < 7:
        raise ValueError("impulse_rider: min_history must be >= 7 (the stencil reaches t - 6)")
    columns = tuple(columns)
    _replay_columns("impulse_rider", columns, _lib.IMPULSE_VALUES, tail=False)
    S, T = _replay_shape(c)
    px = ((o, "open"), (h, "high"), (l, "low"), (c, "close"))
    _replay_panels(px + ((atr, "atr"),), S, T)
    _replay_time(open_time, "open_time", S, T)
    if not isinstance(bench_ts, torch.Tensor) or bench_ts.dtype != torch.int64 or bench_ts.dim() != 1:
        raise ValueError("bench_ts: expected a 1-D int64 tensor of ms timestamps")
    if not isinstance(bench_close, torch.Tensor) or bench_close.dtype != torch.float64 \
            or tuple(bench_close.shape) != tuple(bench_ts.shape):
        raise ValueError(f"bench_close: expected a float64 tensor of shape {tuple(bench_ts.shape)}")
    lens, first_t, _ = _replay_rows(lens, first_t, None, S)
    if not bench_ts.is_cuda and bench_ts.numel() > 1 and bool((bench_ts[1:] < bench_ts[:-1]).any()):
        raise ValueError("bench_ts: must be ascending")   # a host tensor: rejected without a device
    cols, ld_in = _common_pitch([_check_panel(x, n) for x, n in px])
    atr = _check_panel(atr, "atr")
    ts = _check_ts(open_time, "open_time")
    bts = _check_ts(bench_ts, "bench_ts").reshape(-1)
    bc = _check_panel(bench_close.reshape(1, -1), "bench_close").contiguous()
    if check_bench:
        _check_ascending(bts)
    dev = c.device
    lens, first_t, _ = _replay_rows(lens, first_t, None, S, dev)
    p = _replay_struct(_lib.BqImpulseParams, par, ("min_history",))
    status, outs, vals = _replay_outputs(columns, _lib.IMPULSE_VALUES, S, T, dev)
    st = _lib.load().bq_impulse_rider(_ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), ld_in, _ptr(atr),
                                      _row_stride(atr), _ptr(ts), T, _ptr(lens), _ptr(first_t), S, T, _ptr(bts),
                                      _ptr(bc), bts.numel(), ctypes.byref(p), _ptr(status), vals, T,
                                      _stream_handle(None))
    _lib.check(st, "bq_impulse_rider")
    return outs, status


def _check_ascending(bts: torch.Tensor) -> None:
    """bench_ts ascending, else ValueError. One small reduction read back to
    the host; skipped while a graph is being captured (no host sync there:
    the captured caller vouches for its benchmark frame)."""
    if bts.numel() < 2 or torch.cuda.is_current_stream_capturing():
        return
    if bool((bts[1:] < bts[:-1]).any()):
        raise ValueError("bench_ts: must be ascending")


@device_entry
def bb_stable(bb_upper: torch.Tensor, bb_mid: torch.Tensor, bb_lower: torch.Tensor, n: int = 8,
              max_change_pct: float = 20.0, *, first_t=None, lens=None, change: bool = True):
    """LadderDeployer._bb_stable(n, max_change_pct) at every prefix t
    (strategies/grid/ladder_deployer.py:42-56; bq_bb_stable) on
    df.iloc[first_t[s]:t + 1]. Panels [S, T] float64, unit stride along T,
    any row pitch. Returns (stable bool [S, T], change_pct [S, T] float64 —
    NaN where the method returns before computing it — or None with
    change=False)."""
    if not 1 <= int(n) <= _lib.BB_STABLE_MAX_N:
        raise ValueError(f"bb_stable: n must be in 1..{_lib.BB_STABLE_MAX_N}, got {n}")
    S, T = _replay_shape(bb_mid, "bb_mid")
    bb = ((bb_upper, "bb_upper"), (bb_mid, "bb_mid"), (bb_lower, "bb_lower"))
    _replay_panels(bb, S, T)
    lens, first_t, _ = _replay_rows(lens, first_t, None, S)
    cols, ld_in = _common_pitch([_check_panel(x, nm) for x, nm in bb])
    dev = bb_mid.device
    lens, first_t, _ = _replay_rows(lens, first_t, None, S, dev)
    stable = torch.empty((S, T), dtype=torch.bool, device=dev)
    chg = torch.empty((S, T), dtype=torch.float64, device=dev) if change else None
    st = _lib.load().bq_bb_stable(_ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), ld_in, _ptr(lens), _ptr(first_t), S, T,
                                  int(n), float(max_change_pct), _ptr(stable), _ptr(chg), T, _stream_handle(None))
    _lib.check(st, "bq_bb_stable")
    return stable, chg


TOP_GAINER_DEFAULTS = dict(   # TopGainerEarlyMomentum's class attributes (:42-57, :64-66)
    lookback_high=48, volume_window=32, min_history=56, full_extension_bars=96, min_candle_return=0.01,
    max_candle_return=0.10, min_return_1h=0.05, min_return_2h=0.08, min_return_6h=0.07, max_return_1h=0.20,
    max_extension=0.50, min_short_extension_cap=0.25, min_volume_ratio=1.75, min_range_position=0.75,
    max_upper_wick=0.30, atr_stop_mult=2.2, min_stop_loss_pct=1.5, max_stop_loss_pct=2.0)
_TG_INT_PARAMS = ("lookback_high", "volume_window", "min_history", "full_extension_bars")


@device_entry
def top_gainer_entry(o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, v: torch.Tensor,
                     qv: torch.Tensor | None = None, atr: torch.Tensor | None = None, *,
                     risk_ok: torch.Tensor | None = None, first_t=None, lens=None, columns=_lib.TGE_VALUES,
                     **thresholds):
    """TopGainerEarlyMomentum's features, breakout gate and two-close
    confirmation at every candle, one pass (strategies/top_gainer_early_momentum.py
    :91-253, :363-406; bq_top_gainer_entry): column t of row s = the
    reference on df.iloc[first_t[s]:t + 1]. Panels [S, T] float64 with unit
    stride along T and any row pitch; qv None: the reference's volume * close
    fall-backs; atr None: 0.0; risk_ok [S, T] bool (_risk_profile_allows per
    candle; None: allowed). Returns (status uint8, entry uint8, score,
    stop_loss_pct, values): status / entry are _lib.TGE_REASONS codes
    (TGE_NO_FRAME where t >= lens[s]); values maps each name of `columns` (a
    subset of _lib.TGE_VALUES; others are not written) to [S, T] float64,
    NaN where the feature status is not ready; score / stop_loss_pct [S, T]
    are UNROUNDED — the reference's round_numbers(.., 4) is the host's step —
    and NaN except where status is 0 or risk_rejected. thresholds:
    TOP_GAINER_DEFAULTS' keys."""
    par = _replay_params("top_gainer_entry", TOP_GAINER_DEFAULTS, thresholds, noun="thresholds")
    if int(par["min_history"]) < 25:
        raise ValueError("top_gainer_entry: min_history must be >= 25 (the returns reach t - 24)")
    for k in ("lookback_high", "volume_window", "full_extension_bars"):
        if not 1 <= int(par[k]) <= _lib.TGE_MAX_LOOKBACK:
            raise ValueError(f"top_gainer_entry: {k} must be in 1..{_lib.TGE_MAX_LOOKBACK}, got {par[k]}")
    columns = tuple(columns)
    _replay_columns("top_gainer_entry", columns, _lib.TGE_VALUES, tail=False)
    S, T = _replay_shape(c)
    named = [(o, "open"), (h, "high"), (l, "low"), (c, "close"), (v, "volume")]
    named += [(x, n) for x, n in ((qv, "quote_volume"), (atr, "atr")) if x is not None]
    _replay_panels(named, S, T)
    risk = [(risk_ok, "risk_ok")] if risk_ok is not None else []
    _replay_flags(risk, S, T)
    lens, first_t, _ = _replay_rows(lens, first_t, None, S)
    cols, ld_in = _common_pitch([_check_panel(x, n) for x, n in named[:5]])
    qv = _check_panel(qv, "quote_volume") if qv is not None else None
    atr = _check_panel(atr, "atr") if atr is not None else None
    if risk:
        (risk_ok,) = _replay_flags(risk, S, T, dev=True)   # on its own row pitch
    dev = c.device
    lens, first_t, _ = _replay_rows(lens, first_t, None, S, dev)
    p = _replay_struct(_lib.BqTopGainerParams, par, _TG_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.TGE_VALUES, S, T, dev)
    entry = torch.empty_like(status)
    sc = torch.empty((S, T), dtype=torch.float64, device=dev)
    sl = torch.empty_like(sc)
    st = _lib.load().bq_top_gainer_entry(
        _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), ld_in, _ptr(qv),
        _row_stride(qv) if qv is not None else T, _ptr(atr), _row_stride(atr) if atr is not None else T,
        _ptr(risk_ok), _row_stride(risk_ok) if risk_ok is not None else T, _ptr(lens), _ptr(first_t), S, T,
        ctypes.byref(p), _ptr(status), _ptr(entry), _ptr(sc), _ptr(sl), vals, T, _stream_handle(None))
    _lib.check(st, "bq_top_gainer_entry")
    return status, entry, sc, sl, outs


SWEEP_DEFAULTS = dict(   # LiquidationSweepPump's class attributes (:94-101); min_frame: :314
    min_momentum_atr=0.75, max_momentum_atr=3.0, min_close_location=0.70, min_frame=48 + 6 + 2)


@device_entry
def sweep_select(cols, score_cross: torch.Tensor, *, route_ok: torch.Tensor | None = None, first_t=None, lens=None,
                 symbol_rank: torch.Tensor | None = None, t_range: tuple[int, int] | None = None,
                 rank_score: bool = True, out: dict | None = None, **thresholds):
    """LiquidationSweepPump's candidate gate and the cohort winner per candle
    (strategies/liquidation_sweep_pump.py:271-343, :78-81; bq_sweep_select).
    cols: the 13 [S, T] float64 columns of _lib.SW_COLUMNS, in that order (unit
    stride along T, any common row pitch); score_cross [S, T] bool; route_ok
    [S, T] bool (None: allowed); symbol_rank [S] int32 on the device (None:
    the row index); t_range (t_lo, t_hi): the trigger-candle columns to
    decide (None: all). Returns (status uint8 [S, T], rank_score float64
    [S, T] or None, winner int64 [T], winner_score float64 [T]); columns
    outside t_range are left as allocated (uninitialised), or as `out` holds
    them: out = {"status", "rank_score", "winner", "winner_score"} reuses the
    caller's tensors ([S, T] with one row pitch; [T]). Large panels get their
    [S, T] outputs on enrich_outputs' padded pitch. thresholds:
    SWEEP_DEFAULTS' keys."""
    par = _replay_params("sweep_select", SWEEP_DEFAULTS, thresholds, noun="thresholds")
    cols = list(cols)
    if len(cols) != len(_lib.SW_COLUMNS):
        raise ValueError(f"sweep_select: expected the {len(_lib.SW_COLUMNS)} columns {_lib.SW_COLUMNS}")
    S, T = _replay_shape(cols[0], _lib.SW_COLUMNS[0])
    named = list(zip(cols, _lib.SW_COLUMNS))
    _replay_panels(named, S, T)
    masks = [(score_cross, "score_cross")] + ([(route_ok, "route_ok")] if route_ok is not None else [])
    masks = _replay_flags(masks, S, T, dev=True)   # each on its own row pitch
    score_cross, route_ok = masks[0], (masks[1] if route_ok is not None else None)
    if symbol_rank is not None and (not isinstance(symbol_rank, torch.Tensor) or symbol_rank.dtype != torch.int32
                                    or symbol_rank.numel() != S or not symbol_rank.is_cuda):
        raise ValueError(f"symbol_rank: expected an int32 CUDA tensor of {S} entries")
    t_lo, t_hi = (0, T) if t_range is None else (int(t_range[0]), int(t_range[1]))
    if not 0 <= t_lo <= t_hi <= T:
        raise ValueError(f"t_range: expected 0 <= t_lo <= t_hi <= {T}, got {(t_lo, t_hi)}")
    lens, first_t, _ = _replay_rows(lens, first_t, None, S)
    cols, ld_in = _common_pitch([_check_panel(x, n) for x, n in named])
    dev = cols[0].device
    lens, first_t, _ = _replay_rows(lens, first_t, None, S, dev)
    if symbol_rank is not None:
        symbol_rank = symbol_rank.reshape(S).contiguous()
    p = _replay_struct(_lib.BqSweepParams, par, ("min_frame",))
    if out is None:
        pad = ENRICH_ROW_PAD if S >= 1024 and T >= 1024 else 0
        status = torch.empty((S, T + pad), dtype=torch.uint8, device=dev)[:, :T]
        rs = torch.empty((S, T + pad), dtype=torch.float64, device=dev)[:, :T] if rank_score else None
        winner = torch.empty((T,), dtype=torch.int64, device=dev)
        wscore = torch.empty((T,), dtype=torch.float64, device=dev)
    else:
        status, rs, winner, wscore = out["status"], out.get("rank_score"), out["winner"], out["winner_score"]
        ok = (status.dtype == torch.uint8 and tuple(status.shape) == (S, T) and (T <= 1 or status.stride(1) == 1)
              and winner.dtype == torch.int64 and winner.numel() == T and winner.is_contiguous()
              and wscore.dtype == torch.float64 and wscore.numel() == T and wscore.is_contiguous()
              and (rs is None or (rs.dtype == torch.float64 and tuple(rs.shape) == (S, T)
                                  and (T <= 1 or rs.stride(1) == 1) and _row_stride(rs) == _row_stride(status))))
        if not ok:
            raise ValueError("sweep_select: out tensors do not match the panel (dtype, shape or row pitch)")
    lib = _lib.load()
    work = torch.empty((max(int(lib.bq_sweep_select_workspace(S, T)), 8),), dtype=torch.uint8, device=dev)
    st = lib.bq_sweep_select(
        _lib.ptr_array([x.data_ptr() for x in cols]), ld_in, _ptr(score_cross), _row_stride(score_cross),
        _ptr(route_ok), _row_stride(route_ok) if route_ok is not None else T, _ptr(lens), _ptr(first_t),
        _ptr(symbol_rank), S, T, t_lo, t_hi, ctypes.byref(p), _ptr(status), _ptr(rs), _row_stride(status),
        _ptr(winner), _ptr(wscore), _ptr(work), _stream_handle(None))
    _lib.check(st, "bq_sweep_select")
    return status, rs, winner, wscore


RETEST_DEFAULTS = dict(   # GradualGainerRetest's class attributes (:78-85)
    watch_ms=8 * 3_600_000, min_history=100, breakout_lookback=8, support_factor=1 - 0.5 / 100,
    pullback_factor=1 - 0.04)


@device_entry
def retest_replay(o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, ema: torch.Tensor,
                  open_time: torch.Tensor, leader: torch.Tensor, risk_ok: torch.Tensor | None = None, *,
                  state=None, first_t=None, lens=None, from_t=None, detail: bool = True, level: bool = True,
                  **params):
    """GradualGainerRetest.signal()'s watchlist state machine replayed over
    the panel (strategies/gradual_gainer_retest.py:222-308; bq_retest_replay):
    column t of row s = the method on the message whose frame is
    df.iloc[first_t[s]:t + 1], after the messages of all earlier candles;
    candles from_t[s] .. lens[s] - 1 are replayed. Panels [S, T] float64 with
    unit stride along T and any row pitch (ema: the frame's EMA20 column, read
    at t - 1), open_time [S, T] int64 ms, strictly ascending within a row's
    frame; leader / risk_ok [S, T] bool (risk_ok None: always allowed).
    state: None (start idle, discard) or the (active uint8, started int64,
    level float64) [S] tensors, updated in place. Returns (event uint8,
    detail uint8 or None, level float64 or None), each [S, T] (_lib.BQ_RT_*).
    params: RETEST_DEFAULTS' keys (the two factors formed in Python floats)."""
    par = _replay_params("retest_replay", RETEST_DEFAULTS, params)
    L, mh = int(par["breakout_lookback"]), int(par["min_history"])
    if not 1 <= L <= _lib.RETEST_MAX_LOOKBACK or L >= mh:
        raise ValueError(f"retest_replay: breakout_lookback must be in 1..{_lib.RETEST_MAX_LOOKBACK} and below "
                         f"min_history ({mh}), got {L}")
    if int(par["watch_ms"]) < 0:
        raise ValueError("retest_replay: watch_ms must be >= 0")
    S, T = _replay_shape(c)
    px = ((o, "open"), (h, "high"), (l, "low"), (c, "close"), (ema, "ema"))
    _replay_panels(px, S, T)
    _replay_time(open_time, "open_time", S, T)
    flags = [(leader, "leader")] + ([(risk_ok, "risk_ok")] if risk_ok is not None else [])
    _replay_flags(flags, S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    sa, ss, sl = _replay_state(state, ("active", "started", "level"), (torch.uint8, torch.int64, torch.float64), S)
    cols, ld_in = _common_pitch([_check_panel(x, n) for x, n in px])
    ts = _check_ts(open_time, "open_time")
    _replay_on_device("leader / risk_ok / state", [f for f, _ in flags] + [sa, ss, sl])
    flags, ld_b = _replay_flags(flags, S, T, dev=True, pitch=True)
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _lib.BqRetestParams(int(par["watch_ms"]), mh, L, float(par["support_factor"]), float(par["pullback_factor"]))
    event = torch.empty((S, T), dtype=torch.uint8, device=dev)
    det = torch.empty((S, T), dtype=torch.uint8, device=dev) if detail else None
    lvl = torch.empty((S, T), dtype=torch.float64, device=dev) if level else None
    st = _lib.load().bq_retest_replay(_ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), ld_in,
                                      _ptr(ts), T, _ptr(flags[0]), _ptr(flags[1] if risk_ok is not None else None),
                                      ld_b, _ptr(lens), _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(sa),
                                      _ptr(ss), _ptr(sl), _ptr(event), _ptr(det), _ptr(lvl), T, _stream_handle(None))
    _lib.check(st, "bq_retest_replay")
    return event, det, lvl


SPIKE_FADE_DEFAULTS = dict(   # FailedSpikeFade's class attributes (:42-43)
    window_bars=8, ext_factor=1 + 0.06)


@device_entry
def spike_fade_replay(o: torch.Tensor, h: torch.Tensor, c: torch.Tensor, open_time: torch.Tensor,
                      source_ok: torch.Tensor, src_market: torch.Tensor | None = None,
                      fail_market: torch.Tensor | None = None, *, state=None, first_t=None, lens=None, from_t=None,
                      detail: bool = True, bars: bool = True, **params):
    """FailedSpikeFade.signal()'s pending-spike state machine replayed over
    the panel (strategies/failed_spike_fade.py:596-695; bq_spike_fade_replay):
    column t of row s = the method on the message whose frame is
    df.iloc[first_t[s]:t + 1], after the messages of all earlier candles;
    candles max(from_t[s], first_t[s]) .. lens[s] - 1 are replayed. Panels
    [S, T] float64 with unit stride along T and any row pitch, open_time
    [S, T] int64 ms, strictly ascending within a row's frame; source_ok [S, T]
    bool: source_spike_allows of the frame ending at t. src_market /
    fail_market: source_market_allows / failure_market_allows per candle,
    bool [S, T] or [T] (one row shared by all symbols; None: always allowed).
    state: None (start idle, discard) or the (active uint8, open_time int64,
    high float64, close float64) [S] tensors, updated in place. Returns
    (event uint8, detail uint8 or None, bars uint8 or None), each [S, T]
    (_lib.BQ_FS_*). params: SPIKE_FADE_DEFAULTS' keys (ext_factor formed in
    Python floats)."""
    par = _replay_params("spike_fade_replay", SPIKE_FADE_DEFAULTS, params)
    W, ef = int(par["window_bars"]), float(par["ext_factor"])
    if not 1 <= W <= _lib.SPIKEFADE_MAX_WINDOW:
        raise ValueError(f"spike_fade_replay: window_bars must be in 1..{_lib.SPIKEFADE_MAX_WINDOW}, got {W}")
    if not math.isfinite(ef):
        raise ValueError(f"spike_fade_replay: ext_factor must be finite, got {ef}")
    S, T = _replay_shape(c)
    px = ((o, "open"), (h, "high"), (c, "close"))
    _replay_panels(px, S, T)
    _replay_time(open_time, "open_time", S, T)
    _replay_flags([(source_ok, "source_ok")], S, T)
    masks = [(m, name) for m, name in ((src_market, "src_market"), (fail_market, "fail_market")) if m is not None]
    for m, name in masks:   # written out: a gate may be one [T] row shared by all symbols
        if not isinstance(m, torch.Tensor) or m.dtype != torch.bool or tuple(m.shape) not in ((S, T), (T,)):
            raise ValueError(f"{name}: expected a bool tensor of shape {(S, T)} or {(T,)}")
    shared = [m.dim() == 1 for m, _ in masks]
    if len(set(shared)) > 1:
        raise ValueError("src_market / fail_market: both [S, T] or both [T] (they share one row stride)")
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    sa, so, sh, sc = _replay_state(state, ("active", "open_time", "high", "close"),
                                   (torch.uint8, torch.int64, torch.float64, torch.float64), S)
    cols, ld_in = _common_pitch([_check_panel(x, n) for x, n in px])
    ts = _check_ts(open_time, "open_time")
    _replay_on_device("source_ok / src_market / fail_market / state",
                      [source_ok] + [m for m, _ in masks] + [sa, so, sh, sc])
    (source_ok,) = _replay_flags([(source_ok, "source_ok")], S, T, dev=True)   # on its own row pitch
    if not masks:
        ld_m = T
    elif shared[0]:
        masks, ld_m = [m.contiguous() for m, _ in masks], 0
    else:
        masks, ld_m = _replay_flags(masks, S, T, dev=True, pitch=True)
    masks = iter(masks)
    sm = next(masks) if src_market is not None else None
    fm = next(masks) if fail_market is not None else None
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _lib.BqSpikeFadeParams(W, ef)
    event = torch.empty((S, T), dtype=torch.uint8, device=dev)
    det = torch.empty((S, T), dtype=torch.uint8, device=dev) if detail else None
    brs = torch.empty((S, T), dtype=torch.uint8, device=dev) if bars else None
    st = _lib.load().bq_spike_fade_replay(_ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), ld_in, _ptr(ts), T,
                                          _ptr(source_ok), _row_stride(source_ok), _ptr(sm), _ptr(fm), ld_m,
                                          _ptr(lens), _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(sa),
                                          _ptr(so), _ptr(sh), _ptr(sc), _ptr(event), _ptr(det), _ptr(brs), T,
                                          _stream_handle(None))
    _lib.check(st, "bq_spike_fade_replay")
    return event, det, brs


SPIKE_FRAME_FLOAT = ("volume_cluster_min_ratio", "price_break_base_threshold")
SPIKE_FRAME_COLUMNS = _lib.SPIKE_FRAMES_OUT + SPIKE_FRAME_FLOAT
SPIKE_FRAMES_MAX_T = _lib.SPIKE_FRAMES_MAX_T   # candles per panel row: a frame's sorted prefix lives in LDS


def spike_frames_params(params) -> "_lib.BqSpikeFramesParams":
    """bq_spike_frames_params from a strategies.SpikeParams (or any object with
    its attributes), checked against the kernel's range: ValueError outside it."""
    mode = getattr(params, "volume_cluster_label_mode", "last")
    if mode not in _SPIKE_MODES:
        raise ValueError(f"spike_frames: volume_cluster_label_mode must be one of {sorted(_SPIKE_MODES)}, got {mode!r}")
    vw, cw = int(params.volume_cluster_window), int(params.cumulative_price_window)
    bars = int(params.post_spike_cooldown_bars)
    if not 1 <= vw <= _lib.SPIKE_FRAMES_MAX_WINDOW:
        raise ValueError(f"spike_frames: volume_cluster_window must be in 1..{_lib.SPIKE_FRAMES_MAX_WINDOW}, got {vw}")
    if not 2 <= cw <= _lib.SPIKE_FRAMES_MAX_WINDOW:
        raise ValueError(f"spike_frames: cumulative_price_window must be in 2..{_lib.SPIKE_FRAMES_MAX_WINDOW}, "
                         f"got {cw}")
    if bars >= _lib.SPIKE_FRAMES_MAX_COOLDOWN:
        raise ValueError(f"spike_frames: post_spike_cooldown_bars must be below {_lib.SPIKE_FRAMES_MAX_COOLDOWN} "
                         f"(the cooldown walk scans 64-candle masks), got {bars}")
    if int(params.volume_cluster_min_count) < 0:
        raise ValueError("spike_frames: volume_cluster_min_count must not be negative")
    floats = {k: float(getattr(params, k)) for k in (
        "cumulative_price_threshold", "body_size_pct_min", "volume_cluster_min_ratio", "price_break_base_threshold",
        "volume_quantile", "price_base_floor_quantile", "min_volume_ratio", "min_price_abs_floor")}
    for k, val in floats.items():
        if not math.isfinite(val):
            raise ValueError(f"spike_frames: {k} must be finite, got {val}")
    for k in ("volume_quantile", "price_base_floor_quantile"):
        if not 0.0 <= floats[k] <= 1.0:
            raise ValueError(f"spike_frames: {k} must lie in [0, 1], got {floats[k]}")
    return _lib.BqSpikeFramesParams(vw, int(params.volume_cluster_min_count), cw, _SPIKE_MODES[mode],
                                    int(bool(params.require_both_patterns)), int(bool(params.require_bullish_spike)),
                                    bars, 0, *floats.values())


def spike_frames_cap(params, frame_cap) -> "_lib.BqSpikeFramesCap":
    """bq_spike_frames_cap from a frame_cap and the strategies.SpikeParams attributes that only the frame-local
    columns need, checked against the kernel's range: ValueError outside it."""
    lo, hi = _lib.SPIKE_FRAMES_MIN_CAP, SPIKE_FRAMES_MAX_T
    if isinstance(frame_cap, bool) or not isinstance(frame_cap, int) or not lo <= frame_cap <= hi:
        raise ValueError(f"spike_frames: frame_cap must be an int in {lo}..{hi} (or None: no cap), got {frame_cap!r}")
    bw, aw = int(params.base_window), int(params.accel_volume_deriv_window)
    if not (1 <= bw <= _lib.SPIKE_FRAMES_MAX_WINDOW and 1 <= aw <= _lib.SPIKE_FRAMES_MAX_WINDOW):
        raise ValueError(f"spike_frames: base_window and accel_volume_deriv_window must be in "
                         f"1..{_lib.SPIKE_FRAMES_MAX_WINDOW} under a frame_cap, got {(bw, aw)}")
    q = float(params.price_break_dynamic_q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"spike_frames: price_break_dynamic_q must lie in [0, 1], got {q}")
    return _lib.BqSpikeFramesCap(frame_cap, bw, aw, 0, q)


@device_entry
def spike_frames(cols: dict, params, *, first_t=None, lens=None, from_t=None, aligned: bool = False,
                 columns=SPIKE_FRAME_COLUMNS, frame_cap: int | None = None) -> dict[str, torch.Tensor]:
    """FailedSpikeFade.latest_signal() of every frame of a row
    (strategies/failed_spike_fade.py:229-594; bq_spike_frames): column t of
    row s = the method on a fresh instance whose frame is
    df.iloc[first_t[s]:t + 1] (RangeIndex); candles max(from_t[s],
    first_t[s]) .. lens[s] - 1 are formed. cols: the threshold-independent
    columns of detect(), float64 [S, T] under _lib.SPIKE_FRAMES_IN's names
    (volume_ratio, price_change_abs, dyn_threshold: the forward-filled rolling
    quantile, body_size_pct, cum_pos / cum_neg: the rolling sums of the clipped
    price changes, open, close) and bool [S, T] under _lib.SPIKE_FRAMES_IN_B's
    (the two acceleration flags, upward, downward), each as a frame starting
    at first_t forms it. aligned: column j of an input row holds candle
    first_t[s] + j. params: strategies.SpikeParams. T <= SPIKE_FRAMES_MAX_T
    (the expanding quantile keeps a frame's sorted prefix in LDS): a longer
    panel raises ValueError. Returns {name: [S, T]} for `columns`
    (SPIKE_FRAME_COLUMNS: latest_signal()'s flags as bool, the two calibrated
    thresholds as float64); False / NaN outside the formed candles. Allocates
    by shape, reads nothing back.

    frame_cap = M (64 .. SPIKE_FRAMES_MAX_T; bq_spike_frames_capped): the
    frame of column t is df.iloc[max(first_t[s], t + 1 - M):t + 1] instead, the
    live store's sliding frame; T is then not limited (a frame's keys live in
    LDS, whatever T). cols are still the columns of a frame starting at
    first_t, with two int32 [S, T] columns beside them (_lib.SPIKE_FRAMES_IN_I;
    strategies.spike_frame_columns(cap=True) forms them): dyn_src, the column
    index of dyn_threshold's forward-fill source (-1: none), and close_next,
    the index of the first valid close at or after the column (T: none). The
    kernels restate what is frame-local near each frame's start (the header's
    rule table); deeper rows agree with pandas to running-sum rounding.
    frame_cap >= T is the uncapped call."""
    _replay_columns("spike_frames", columns, SPIKE_FRAME_COLUMNS)
    p = spike_frames_params(params)
    cap = None if frame_cap is None else spike_frames_cap(params, frame_cap)
    missing = [k for k in _lib.SPIKE_FRAMES_IN + _lib.SPIKE_FRAMES_IN_B if k not in cols]
    if missing:
        raise ValueError(f"spike_frames: missing input columns {missing}")
    S, T = _replay_shape(cols["close"])
    if cap is not None and frame_cap >= T:   # no frame slides
        cap = None
    if cap is None and T > SPIKE_FRAMES_MAX_T:
        raise ValueError(f"spike_frames: T = {T} exceeds the cap of {SPIKE_FRAMES_MAX_T} candles per row")
    names_i = _lib.SPIKE_FRAMES_IN_I if cap is not None else ()
    if cap is not None:
        missing = [k for k in names_i if k not in cols]
        if missing:
            raise ValueError(f"spike_frames: missing input columns {missing} (frame_cap needs them)")
        for k in names_i:
            x = cols[k]
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int32:
                raise ValueError(f"{k}: expected dtype int32, got {getattr(x, 'dtype', type(x))}")
            if tuple(x.shape) != (S, T):
                raise ValueError(f"{k}: shape {tuple(x.shape)} != {(S, T)}")
    fin = [(cols[k], k) for k in _lib.SPIKE_FRAMES_IN]
    _replay_panels(fin, S, T)
    bflags = [(cols[k], k) for k in _lib.SPIKE_FRAMES_IN_B]
    _replay_flags(bflags, S, T, (torch.bool, torch.uint8))
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    fcols, ld_in = _common_pitch([_check_panel(x, n) for x, n in fin])
    _replay_on_device("spike_frames: flag inputs", [x for x, _ in bflags])
    bcols, ld_b = _replay_flags(bflags, S, T, (torch.bool, torch.uint8), dev=True, pitch=True)
    dev = fcols[0].device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    out = {k: torch.empty((S, T), dtype=torch.float64 if k in SPIKE_FRAME_FLOAT else torch.bool, device=dev)
           for k in SPIKE_FRAME_COLUMNS if k in columns}
    lib = _lib.load()
    if cap is not None:
        _replay_on_device("spike_frames: index inputs", [cols[k] for k in names_i])
        icols = [cols[k].contiguous() for k in names_i]
        nbytes = int(lib.bq_spike_frames_capped_workspace(S, T))
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        st = lib.bq_spike_frames_capped(
            _lib.ptr_array([x.data_ptr() for x in fcols]), ld_in, _lib.ptr_array([x.data_ptr() for x in bcols]), ld_b,
            _lib.ptr_array([x.data_ptr() for x in icols]), T, int(bool(aligned)), _ptr(lens), _ptr(first_t),
            _ptr(from_t), S, T, ctypes.byref(p), ctypes.byref(cap), _ptr(ws), nbytes,
            _ptr(out.get("volume_cluster_min_ratio")), _ptr(out.get("price_break_base_threshold")),
            _lib.ptr_array([out[k].data_ptr() if k in out else 0 for k in _lib.SPIKE_FRAMES_OUT]), T,
            _stream_handle(None))
        _lib.check(st, "bq_spike_frames_capped")
        return out
    nbytes = int(lib.bq_spike_frames_workspace(S, T))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    st = lib.bq_spike_frames(
        _lib.ptr_array([x.data_ptr() for x in fcols]), ld_in, _lib.ptr_array([x.data_ptr() for x in bcols]), ld_b,
        int(bool(aligned)), _ptr(lens), _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(ws), nbytes,
        _ptr(out.get("volume_cluster_min_ratio")), _ptr(out.get("price_break_base_threshold")),
        _lib.ptr_array([out[k].data_ptr() if k in out else 0 for k in _lib.SPIKE_FRAMES_OUT]), T,
        _stream_handle(None))
    _lib.check(st, "bq_spike_frames")
    return out


PRICE_TRACKER_DEFAULTS = dict(   # PriceTracker.signal()'s constants and class attributes (:34-35, :59-63, :177-239)
    min_history=30, tail_rows=5, span_fast=9, span_slow=21, rsi_max=30.0, macd_max=0.0, mfi_max=20.0, w_rsi=0.35,
    w_mfi=0.35, w_macd=0.3, macd_scale=100.0, context_weight=0.35, risk_weight=0.35, support_weight=0.2,
    min_followthrough=-0.2, max_risk=0.6, min_confidence=0.5, cooldown_ms=12 * 300_000)
_PT_INT_PARAMS = ("min_history", "tail_rows", "span_fast", "span_slow", "cooldown_ms")


@device_entry
def price_tracker_replay(c: torch.Tensor, rsi: torch.Tensor, macd: torch.Tensor, mfi: torch.Tensor,
                         close_time: torch.Tensor, symbol_rs: torch.Tensor, ctx: torch.Tensor,
                         ctx_ok: torch.Tensor | None = None, *, h: torch.Tensor | None = None,
                         l: torch.Tensor | None = None, v: torch.Tensor | None = None,
                         trend_score: torch.Tensor | None = None, state=None, first_t=None, lens=None, from_t=None,
                         detail: bool = True, columns=_lib.PT_VALUES, **params):
    """PriceTracker.signal() replayed over the panel
    (strategies/coinrule/price_tracker.py:165-324; bq_price_tracker_replay):
    column t of row s = the method on the message whose frame is
    df.iloc[first_t[s]:t + 1], after the messages of all earlier candles;
    candles max(from_t[s], first_t[s]) .. lens[s] - 1 are replayed. c / rsi /
    macd / mfi (and h / l / v, read by the null test only; None: no NaN in
    them) [S, T] float64 with unit stride along T and any row pitch,
    mfi[s, t] = Indicators.mfi of the frame ending at t; close_time [S, T]
    int64 ms, strictly ascending within a row's frame. trend_score [S, T] or
    None: the EMA 9 / 21 score formed in the pass. symbol_rs float64 [S] or
    [S, T]; ctx float64 [4, Tc] (_lib.PT_CTX_ROWS), Tc 1 or T, and ctx_ok
    bool / uint8 [Tc] (None: present), on the device. state: None (no entry,
    discard) or the (has uint8, last_close_time int64) [S] tensors, updated in
    place. Returns (status uint8 [S, T] (_lib.BQ_PT_*), detail uint8 [S, T] or
    None, {name: float64 [S, T]} for `columns`, a subset of _lib.PT_VALUES,
    NaN where the method did not reach them). params: PRICE_TRACKER_DEFAULTS'
    keys (cooldown_ms 0: strategy_cooldowns is None)."""
    par = _replay_params("price_tracker_replay", PRICE_TRACKER_DEFAULTS, params, _PT_INT_PARAMS)
    if int(par["min_history"]) < 1 or not 1 <= int(par["tail_rows"]) <= _lib.PT_MAX_TAIL_ROWS:
        raise ValueError(f"price_tracker_replay: min_history >= 1 and tail_rows in 1..{_lib.PT_MAX_TAIL_ROWS}")
    if int(par["span_fast"]) < 1 or int(par["span_slow"]) < 1 or int(par["cooldown_ms"]) < 0:
        raise ValueError("price_tracker_replay: spans must be >= 1 and cooldown_ms >= 0")
    if float(par["rsi_max"]) == 0.0 or float(par["mfi_max"]) == 0.0:
        raise ValueError("price_tracker_replay: rsi_max and mfi_max divide local_score's terms: not 0")
    _replay_columns("price_tracker_replay", columns, _lib.PT_VALUES)
    S, T = _replay_shape(c)
    px = [(c, "close")] + [(x, n) for x, n in ((h, "high"), (l, "low"), (v, "volume")) if x is not None]
    ind = [(rsi, "rsi"), (macd, "macd"), (mfi, "mfi")]
    opt = [(trend_score, "trend_score")] if trend_score is not None else []
    _replay_panels(px + ind + opt, S, T)
    _replay_time(close_time, "close_time", S, T)
    if (not isinstance(symbol_rs, torch.Tensor) or symbol_rs.dtype != torch.float64
            or tuple(symbol_rs.shape) not in ((S,), (S, T))):
        raise ValueError(f"symbol_rs: expected a float64 tensor of shape {(S,)} or {(S, T)}")
    ctx, ctx_ok, Tc, ld_ctx = _replay_ctx(ctx, ctx_ok, _lib.PT_CTX_ROWS, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    sh, sl = _replay_state(state, ("has", "last_close_time"), (torch.uint8, torch.int64), S)
    pxs, ld_px = _common_pitch([_check_panel(x, n) for x, n in px])
    inds, ld_ind = _common_pitch([_check_panel(x, n) for x, n in ind])
    tr = _check_panel(trend_score, "trend_score") if trend_score is not None else None
    ct = _check_ts(close_time, "close_time")
    _replay_on_device("symbol_rs / ctx / ctx_ok / state", [symbol_rs, ctx, ctx_ok, sh, sl])
    if symbol_rs.dim() == 2:
        symbol_rs = _check_panel(symbol_rs, "symbol_rs")
        ld_rs = _row_stride(symbol_rs)
    else:
        symbol_rs, ld_rs = symbol_rs.contiguous(), 0
    cc, rest = pxs[0], iter(pxs[1:])
    hh, ll, vv = (next(rest) if x is not None else None for x in (h, l, v))
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqPriceTrackerParams, par, _PT_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.PT_VALUES, S, T, dev)
    det = torch.empty((S, T), dtype=torch.uint8, device=dev) if detail else None
    st = _lib.load().bq_price_tracker_replay(
        _ptr(cc), _ptr(hh), _ptr(ll), _ptr(vv), ld_px, _ptr(inds[0]), _ptr(inds[1]), _ptr(inds[2]), ld_ind, _ptr(ct), T,
        _ptr(tr), _row_stride(tr) if tr is not None else T, _ptr(symbol_rs), ld_rs, _ptr(ctx), ld_ctx, _ptr(ctx_ok), Tc,
        _ptr(lens), _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(sh), _ptr(sl), _ptr(status), _ptr(det),
        vals, T, _stream_handle(None))
    _lib.check(st, "bq_price_tracker_replay")
    return status, det, outs


MEAN_REVERSION_DEFAULTS = dict(   # MeanReversionFade's class attributes (strategies/mean_reversion_fade.py:52-73)
    rsi_window=14, volume_ma_window=20, atr_ma_window=20, ema_fast=20, ema_slow=50, rsi_short_min=76.0,
    volume_ratio_min=0.8, atr_spike_max=2.2, atr_stop_mult=2.0, max_entry_stop_loss_pct=1.5, max_trend_score=0.005,
    max_market_stress=0.25, max_gap=0.02, max_symbol_atr_pct=0.03, min_wick_ratio=0.0)
_MR_INT_PARAMS = ("rsi_window", "volume_ma_window", "atr_ma_window", "ema_fast", "ema_slow")
_MR_SYM = (("ok", (torch.uint8, torch.bool)), ("atr_pct", (torch.float64,)), ("trend_score", (torch.float64,)),
           ("regime", (torch.uint8,)), ("transition", (torch.uint8,)))


@device_entry
def mean_reversion_replay(o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, v: torch.Tensor,
                          atr: torch.Tensor, bb_upper: torch.Tensor, open_time: torch.Tensor, ctx: torch.Tensor,
                          ctx_ok: torch.Tensor | None = None, *, sym=None, features=None, state=None, first_t=None,
                          lens=None, from_t=None, columns=_lib.MR_VALUES, **params):
    """MeanReversionFade.signal() replayed over the panel
    (strategies/mean_reversion_fade.py:224-300; bq_mean_reversion_replay):
    column t of row s = the method on the message whose frame is
    df_15m.iloc[first_t[s]:t + 1], after the messages of all earlier candles;
    candles max(from_t[s], first_t[s]) .. lens[s] - 1 are replayed. o / h / l /
    c / v / atr (the frame's ATR column) / bb_upper (the bb_high passed to
    signal()) [S, T] float64 with unit stride along T and any row pitch;
    open_time [S, T] int64, strictly ascending within a row's frame. ctx
    float64 [5, Tc] (_lib.MR_CTX_ROWS), Tc 1 or T, and ctx_ok bool / uint8 [Tc]
    (None: present), on the device. sym: None (no symbol has features in the
    snapshot) or the (ok uint8 / bool, atr_pct float64, trend_score float64,
    regime uint8, transition uint8) tensors, all [S] or all [S, T]; regime /
    transition index _lib.MICRO_REGIMES / _lib.MICRO_TRANSITIONS, _lib.MR_NONE
    for None. features: None (formed in the pass over the frame starting at
    first_t) or the (rsi, previous_rsi, volume_ma, atr_ma, trend_score) [S, T]
    float64 tensors. state: None (no entry, discard) or the (has uint8,
    last_open_time int64) [S] tensors, updated in place. Returns (status uint8
    [S, T] (_lib.MR_REASONS' indices), {name: float64 [S, T]} for `columns`, a
    subset of _lib.MR_VALUES, NaN where the method did not reach them).
    params: MEAN_REVERSION_DEFAULTS' keys."""
    par = _replay_params("mean_reversion_replay", MEAN_REVERSION_DEFAULTS, params, _MR_INT_PARAMS)
    if int(par["rsi_window"]) < 1 or int(par["ema_fast"]) < 1 or int(par["ema_slow"]) < 1:
        raise ValueError("mean_reversion_replay: rsi_window and the spans must be >= 1")
    if not all(1 <= int(par[k]) <= _lib.MR_MAX_WINDOW for k in ("volume_ma_window", "atr_ma_window")):
        raise ValueError(f"mean_reversion_replay: volume_ma_window and atr_ma_window in 1..{_lib.MR_MAX_WINDOW}")
    if float(par["rsi_short_min"]) == 100.0:
        raise ValueError("mean_reversion_replay: 100 - rsi_short_min divides the score: not 100")
    _replay_columns("mean_reversion_replay", columns, _lib.MR_VALUES)
    S, T = _replay_shape(c)
    px = [(o, "open"), (h, "high"), (l, "low"), (c, "close"), (v, "volume")]
    ft = _replay_features(features, _lib.MR_VALUES[:_lib.MR_NFEATURES])
    _replay_panels(px + [(atr, "atr"), (bb_upper, "bb_upper")] + ft, S, T)
    _replay_time(open_time, "open_time", S, T)
    ctx, ctx_ok, Tc, ld_ctx = _replay_ctx(ctx, ctx_ok, _lib.MR_CTX_ROWS, T)
    sy, ld_sym = _replay_sym(sym, _MR_SYM, S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    sh, sl = _replay_state(state, ("has", "last_open_time"), (torch.uint8, torch.int64), S)
    pxs, ld_px = _common_pitch([_check_panel(x, n) for x, n in px])
    atr, bb_upper = _check_panel(atr, "atr"), _check_panel(bb_upper, "bb_upper")
    fts, ld_ft = _common_pitch([_check_panel(x, n) for x, n in ft]) if ft else ([], T)
    ot = _check_ts(open_time, "open_time")
    _replay_on_device("ctx / ctx_ok / sym / state", [ctx, ctx_ok, *sy, sh, sl])
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqMeanReversionParams, par, _MR_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.MR_VALUES, S, T, dev)
    feats = _lib.ptr_array([x.data_ptr() for x in fts]) if fts else None
    st = _lib.load().bq_mean_reversion_replay(
        _ptr(pxs[0]), _ptr(pxs[1]), _ptr(pxs[2]), _ptr(pxs[3]), _ptr(pxs[4]), ld_px, _ptr(atr), _row_stride(atr),
        _ptr(bb_upper), _row_stride(bb_upper), _ptr(ot), T, feats, ld_ft, _ptr(ctx), ld_ctx, _ptr(ctx_ok), Tc,
        _ptr(sy[0]), _ptr(sy[1]), _ptr(sy[2]), _ptr(sy[3]), _ptr(sy[4]), ld_sym, _ptr(lens), _ptr(first_t),
        _ptr(from_t), S, T, ctypes.byref(p), _ptr(sh), _ptr(sl), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_mean_reversion_replay")
    return status, outs


RANGE_FADE_DEFAULTS = dict(   # RangeBbRsiMeanReversion's class attributes (range_bb_rsi_mean_reversion.py:37-51)
    min_candles=40, adx_window=14, zscore_window=20, adx_max=32.0, long_rsi_max=35.0, short_rsi_min=65.0,
    long_zscore_max=-2.0, short_zscore_min=2.0, band_touch_tolerance=0.002, max_market_stress=0.35,
    max_symbol_atr_pct=0.04, max_symbol_bb_width=0.08, min_rejection_wick_frac=0.30, long_close_position_min=0.55,
    short_close_position_max=0.45)
_RF_INT_PARAMS = ("min_candles", "adx_window", "zscore_window")
_RF_SYM = (("ok", (torch.uint8, torch.bool)), ("micro_regime", (torch.uint8,)), ("micro_transition", (torch.uint8,)),
           ("atr_pct", (torch.float64,)), ("bb_width", (torch.float64,)))


@device_entry
def range_fade_replay(o: torch.Tensor, h: torch.Tensor, l: torch.Tensor, c: torch.Tensor, v: torch.Tensor,
                      rsi: torch.Tensor, bb_upper: torch.Tensor, bb_mid: torch.Tensor, bb_lower: torch.Tensor,
                      ctx: torch.Tensor, ctx_ok: torch.Tensor | None = None, *, sym=None, features=None, first_t=None,
                      lens=None, from_t=None, columns=_lib.RF_VALUES, **params):
    """RangeBbRsiMeanReversion.signal() replayed over the panel
    (strategies/range_bb_rsi_mean_reversion.py:202-274; bq_range_fade_replay):
    column t of row s = the method on the message whose frame is
    df_15m.iloc[first_t[s]:t + 1]; candles max(from_t[s], first_t[s]) ..
    lens[s] - 1 are replayed. The strategy keeps no cooldown entry: no state.
    o / h / l / c / v / rsi (the enriched frame's columns; v only feeds the
    null gate) / bb_upper / bb_mid / bb_lower (the bb_high, bb_mid, bb_low
    passed to signal(), as the caller rounds them) [S, T] float64 with unit
    stride along T and any row pitch; current_price is the candle's close. ctx
    float64 [3, Tc] (_lib.RF_CTX_ROWS; market_regime an index into
    _lib.MARKET_REGIMES, _lib.MR_NONE for None), Tc 1 or T, and ctx_ok bool /
    uint8 [Tc] (None: present), on the device. sym: None (no symbol has
    features in the snapshot) or the (ok uint8 / bool, micro_regime uint8,
    micro_transition uint8, atr_pct float64, bb_width float64) tensors, all [S]
    or all [S, T]; the codes index _lib.MICRO_REGIMES / _lib.MICRO_TRANSITIONS,
    _lib.MR_NONE for None. features: None (adx and zscore are formed in the
    pass over the frame starting at first_t) or the (adx, zscore) [S, T]
    float64 tensors. Returns (status uint8 [S, T] (_lib.RF_REASONS' indices),
    {name: float64 [S, T]} for `columns`, a subset of _lib.RF_VALUES, NaN where
    the method did not reach them). params: RANGE_FADE_DEFAULTS' keys."""
    par = _replay_params("range_fade_replay", RANGE_FADE_DEFAULTS, params, _RF_INT_PARAMS)
    if int(par["min_candles"]) < 1:
        raise ValueError("range_fade_replay: min_candles must be >= 1")
    if not 1 <= int(par["adx_window"]) <= _lib.RF_MAX_ADX_WINDOW:
        raise ValueError(f"range_fade_replay: adx_window in 1..{_lib.RF_MAX_ADX_WINDOW}")
    if not 1 <= int(par["zscore_window"]) <= _lib.RF_MAX_ZSCORE_WINDOW:
        raise ValueError(f"range_fade_replay: zscore_window in 1..{_lib.RF_MAX_ZSCORE_WINDOW}")
    if float(par["adx_max"]) == 0.0 or float(par["long_rsi_max"]) == 0.0:
        raise ValueError("range_fade_replay: adx_max and long_rsi_max divide the score: not 0")
    _replay_columns("range_fade_replay", columns, _lib.RF_VALUES)
    S, T = _replay_shape(c)
    px = [(o, "open"), (h, "high"), (l, "low"), (c, "close"), (v, "volume")]
    bb = [(bb_upper, "bb_upper"), (bb_mid, "bb_mid"), (bb_lower, "bb_lower")]
    ft = _replay_features(features, _lib.RF_VALUES[:_lib.RF_NFEATURES])
    _replay_panels(px + [(rsi, "rsi")] + bb + ft, S, T)
    ctx, ctx_ok, Tc, ld_ctx = _replay_ctx(ctx, ctx_ok, _lib.RF_CTX_ROWS, T)
    sy, ld_sym = _replay_sym(sym, _RF_SYM, S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    pxs, ld_px = _common_pitch([_check_panel(x, n) for x, n in px])
    rsi = _check_panel(rsi, "rsi")
    bbs, ld_bb = _common_pitch([_check_panel(x, n) for x, n in bb])
    fts, ld_ft = _common_pitch([_check_panel(x, n) for x, n in ft]) if ft else ([], T)
    _replay_on_device("ctx / ctx_ok / sym", [ctx, ctx_ok, *sy])
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqRangeFadeParams, par, _RF_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.RF_VALUES, S, T, dev)
    feats = _lib.ptr_array([x.data_ptr() for x in fts]) if fts else None
    st = _lib.load().bq_range_fade_replay(
        _ptr(pxs[0]), _ptr(pxs[1]), _ptr(pxs[2]), _ptr(pxs[3]), _ptr(pxs[4]), ld_px, _ptr(rsi), _row_stride(rsi),
        _ptr(bbs[0]), _ptr(bbs[1]), _ptr(bbs[2]), ld_bb, feats, ld_ft, _ptr(ctx), ld_ctx, _ptr(ctx_ok), Tc,
        _ptr(sy[0]), _ptr(sy[1]), _ptr(sy[2]), _ptr(sy[3]), _ptr(sy[4]), ld_sym, _ptr(lens), _ptr(first_t),
        _ptr(from_t), S, T, ctypes.byref(p), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_range_fade_replay")
    return status, outs


BUY_THE_DIP_DEFAULTS = dict(   # BuyTheDip's class attributes (strategies/coinrule/buy_the_dip.py:34-36) and :67, :159
    lookback_candles=24, lookback_ms=6 * 3_600_000, start_time_ms=1_776_036_060_000, min_change_pct=-5.0,
    max_change_pct=-2.0, ema_span=20)
_DIP_INT_PARAMS = ("lookback_candles", "lookback_ms", "start_time_ms", "ema_span")


def _replay_regime(x, name: str, shapes):
    """x: None (absent) or an int8 code tensor of one of `shapes`."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int8 or tuple(x.shape) not in shapes:
        raise ValueError(f"{name}: expected an int8 tensor of shape {' or '.join(str(s) for s in shapes)}")
    return x


@device_entry
def buy_the_dip_replay(c: torch.Tensor, close_time: torch.Tensor, market_regime: torch.Tensor | None,
                       micro_regime: torch.Tensor | None, *, ema20: torch.Tensor | None = None, first_t=None,
                       lens=None, from_t=None, columns=_lib.DIP_VALUES, **params):
    """BuyTheDip.signal() replayed over the panel
    (strategies/coinrule/buy_the_dip.py:127-243; bq_buy_the_dip_replay): column
    t of row s = the method on the message whose frame is
    df.iloc[first_t[s]:t + 1] with current_price = close[t]; candles
    max(from_t[s], first_t[s]) .. lens[s] - 1 are replayed. c [S, T] float64
    with unit stride along T and any row pitch; close_time [S, T] int64 ms,
    strictly ascending within a row's frame. ema20 [S, T] or None: the frame's
    close.ewm(span=ema_span, adjust=False, min_periods=1).mean() formed in the
    pass. market_regime int8 [1] or [T] (_lib.MARKET_REGIMES codes, negative:
    no context, or None) and micro_regime int8 [S] or [S, T]
    (_lib.MICRO_REGIMES codes, negative: no features, or None), on the device;
    None: no context / no features for any candle. Returns (status uint8
    [S, T] (_lib.BQ_DIP_*), {name: float64 [S, T]} for `columns`, a subset of
    _lib.DIP_VALUES, NaN where the method did not reach them). params:
    BUY_THE_DIP_DEFAULTS' keys."""
    par = _replay_params("buy_the_dip_replay", BUY_THE_DIP_DEFAULTS, params, _DIP_INT_PARAMS)
    if not float(par["min_change_pct"]) < float(par["max_change_pct"]):
        raise ValueError("buy_the_dip_replay: min_change_pct must be below max_change_pct")
    if int(par["lookback_candles"]) < 2 or int(par["lookback_ms"]) <= 0 or int(par["ema_span"]) < 1:
        raise ValueError("buy_the_dip_replay: lookback_candles >= 2 (the prior close), lookback_ms > 0, ema_span >= 1")
    columns = tuple(columns)
    _replay_columns("buy_the_dip_replay", columns, _lib.DIP_VALUES)
    S, T = _replay_shape(c)
    _replay_panels([(c, "close")] + ([(ema20, "ema20")] if ema20 is not None else []), S, T)
    _replay_time(close_time, "close_time", S, T)
    mk = _replay_regime(market_regime, "market_regime", ((1,), (T,)))
    mr = _replay_regime(micro_regime, "micro_regime", ((S,), (S, T)))
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    cc = _check_panel(c, "close")
    em = _check_panel(ema20, "ema20") if ema20 is not None else None
    ct = _check_ts(close_time, "close_time")
    _replay_on_device("market_regime / micro_regime", [mk, mr])
    mk = mk.contiguous() if mk is not None else None
    mr = mr.contiguous() if mr is not None else None
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqBuyTheDipParams, par, _DIP_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.DIP_VALUES, S, T, dev)
    st = _lib.load().bq_buy_the_dip_replay(
        _ptr(cc), _row_stride(cc), _ptr(ct), T, _ptr(em), _row_stride(em) if em is not None else T, _ptr(mk),
        mk.numel() if mk is not None else 1, _ptr(mr), T if mr is not None and mr.dim() == 2 else 0, _ptr(lens),
        _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_buy_the_dip_replay")
    return status, outs


BB_EXTREME_DEFAULTS = dict(   # BBExtremeReversion's class attributes (strategies/coinrule/bb_extreme_reversion.py:50-67)
    lookback=30, rsi_window=2, oversold_rsi=5.0, overbought_rsi=95.0, max_lower_band_position=0.0,
    min_upper_band_position=1.0)
_BBX_INT_PARAMS = ("lookback", "rsi_window")


@device_entry
def bb_extreme_replay(c: torch.Tensor, bb_upper: torch.Tensor, bb_mid: torch.Tensor, bb_lower: torch.Tensor, *,
                      first_t=None, lens=None, from_t=None, columns=_lib.BBX_VALUES, **params):
    """BBExtremeReversion.signal() replayed over the panel, as it runs with
    ENABLED true (strategies/coinrule/bb_extreme_reversion.py:234-285;
    bq_bb_extreme_replay): column t of row s = the method on the message whose
    frame is df.iloc[first_t[s]:t + 1] with current_price = close[t] and the
    bands of candle t; candles max(from_t[s], first_t[s]) .. lens[s] - 1 are
    replayed. c / bb_upper / bb_mid / bb_lower [S, T] float64 with unit stride
    along T and any row pitch. The bands are taken as given: the evaluator's
    round_numbers(.., 6) on bb_spreads is the caller's step. The RSI is
    _compute_rsi's, pandas' rolling mean replayed over each candle's own last
    `lookback` closes, bit for bit. Returns (status uint8 [S, T]
    (_lib.BQ_BBX_*), {name: float64 [S, T]} for `columns`, a subset of
    _lib.BBX_VALUES, NaN where the method did not reach evaluate). params:
    BB_EXTREME_DEFAULTS' keys; rsi_window + 1 > lookback is the method's own
    "not enough candles" branch, not an error."""
    par = _replay_params("bb_extreme_replay", BB_EXTREME_DEFAULTS, params, _BBX_INT_PARAMS)
    if not 1 <= int(par["lookback"]) <= _lib.BBX_MAX_LOOKBACK:
        raise ValueError(f"bb_extreme_replay: lookback in 1..{_lib.BBX_MAX_LOOKBACK}")
    if int(par["rsi_window"]) < 1:
        raise ValueError("bb_extreme_replay: rsi_window must be >= 1")
    columns = tuple(columns)
    _replay_columns("bb_extreme_replay", columns, _lib.BBX_VALUES)
    S, T = _replay_shape(c)
    bb = [(bb_upper, "bb_upper"), (bb_mid, "bb_mid"), (bb_lower, "bb_lower")]
    _replay_panels([(c, "close")] + bb, S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    cc = _check_panel(c, "close")
    bbs, ld_bb = _common_pitch([_check_panel(x, n) for x, n in bb])
    _replay_on_device("close / bb_upper / bb_mid / bb_lower", [cc, *bbs])
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqBbExtremeParams, par, _BBX_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.BBX_VALUES, S, T, dev)
    st = _lib.load().bq_bb_extreme_replay(
        _ptr(cc), _row_stride(cc), _ptr(bbs[0]), _ptr(bbs[1]), _ptr(bbs[2]), ld_bb, _ptr(lens), _ptr(first_t),
        _ptr(from_t), S, T, ctypes.byref(p), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_bb_extreme_replay")
    return status, outs


RS_REVERSAL_DEFAULTS = dict(   # RelativeStrengthReversalRange's class attributes
    window=96, quantile=0.20, avg_return_max=-0.02, rs_min=0.05)   # (strategies/relative_strength_reversal_range.py:38-41)
_RSR_INT_PARAMS = ("window",)


@device_entry
def rs_reversal_replay(volume: torch.Tensor, context_ok: torch.Tensor | None, market_regime: torch.Tensor,
                       average_return: torch.Tensor, features_ok: torch.Tensor | None, rs: torch.Tensor, *,
                       first_t=None, lens=None, from_t=None, columns=_lib.RSR_VALUES, **params):
    """RelativeStrengthReversalRange.signal() replayed over the panel
    (strategies/relative_strength_reversal_range.py:56-101;
    bq_rs_reversal_replay): column t of row s = the method on the message
    whose frame is df.iloc[first_t[s]:t + 1]; candles max(from_t[s],
    first_t[s]) .. lens[s] - 1 are replayed. volume [S, T] float64 with unit
    stride along T and any row pitch. The context of candle t's message, on the
    device, [1] (one context for every candle) or [T]: context_ok bool / uint8
    (None: present), market_regime int8 (_lib.MARKET_REGIMES codes, negative:
    None), average_return float64. The symbol's entry in the context's
    snapshot, [S] or [S, T]: features_ok bool / uint8 (None: present) and rs
    float64, its relative_strength_vs_btc. The volume floor is Series.quantile
    over the frame's last `window` volumes (numpy's two-sided lerp over the
    non-NaN rows, +-inf a value), formed only in the 64-candle steps where a
    candle passes the route. Returns (status uint8 [S, T] (_lib.BQ_RSR_*),
    {name: float64 [S, T]} for `columns`, a subset of _lib.RSR_VALUES, NaN
    where the method did not reach the floor). params: RS_REVERSAL_DEFAULTS'
    keys."""
    par = _replay_params("rs_reversal_replay", RS_REVERSAL_DEFAULTS, params, _RSR_INT_PARAMS)
    if not 1 <= int(par["window"]) <= _lib.RSR_MAX_WINDOW:
        raise ValueError(f"rs_reversal_replay: window in 1..{_lib.RSR_MAX_WINDOW}")
    if not 0.0 <= float(par["quantile"]) <= 1.0:
        raise ValueError("rs_reversal_replay: quantile in [0, 1]")
    columns = tuple(columns)
    _replay_columns("rs_reversal_replay", columns, _lib.RSR_VALUES)
    S, T = _replay_shape(volume)
    _replay_panels([(volume, "volume")], S, T)
    mk = _replay_regime(market_regime, "market_regime", ((1,), (T,)))
    if mk is None:
        raise ValueError("market_regime: expected an int8 tensor of shape (1,) or (T,) (negative codes: None)")
    Tc = int(mk.numel())
    if (not isinstance(average_return, torch.Tensor) or average_return.dtype != torch.float64
            or tuple(average_return.shape) != (Tc,)):
        raise ValueError(f"average_return: expected a float64 tensor of shape {(Tc,)}")
    if context_ok is not None and (not isinstance(context_ok, torch.Tensor)
                                   or context_ok.dtype not in (torch.bool, torch.uint8)
                                   or tuple(context_ok.shape) != (Tc,)):
        raise ValueError(f"context_ok: expected a bool / uint8 tensor of shape {(Tc,)}")
    flags = (torch.bool, torch.uint8)
    if features_ok is None:
        (rsv,), ld_sym = _replay_sym((rs,), (("relative_strength_vs_btc", (torch.float64,)),), S, T)
        fok = None
    else:
        (fok, rsv), ld_sym = _replay_sym((features_ok, rs), (("features_ok", flags),
                                                             ("relative_strength_vs_btc", (torch.float64,))), S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    vv = _check_panel(volume, "volume")
    _replay_on_device("context_ok / market_regime / average_return / features_ok / relative_strength_vs_btc",
                      [context_ok, mk, average_return, fok, rsv])
    cok = context_ok.contiguous() if context_ok is not None else None
    mk, ar = mk.contiguous(), average_return.contiguous()
    dev = volume.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqRsReversalParams, par, _RSR_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.RSR_VALUES, S, T, dev)
    st = _lib.load().bq_rs_reversal_replay(
        _ptr(vv), _row_stride(vv), _ptr(cok), _ptr(mk), _ptr(ar), Tc, _ptr(fok), _ptr(rsv), ld_sym, _ptr(lens),
        _ptr(first_t), _ptr(from_t), S, T, ctypes.byref(p), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_rs_reversal_replay")
    return status, outs


GRID_LADDER_TILE = _lib.GRID_LADDER_TILE   # candles per workgroup tile of bq_grid_ladder_replay
GRID_LADDER_DEFAULTS = dict(   # LadderDeployer's class attributes (strategies/grid/ladder_deployer.py:16-28)
    n=8, max_change_pct=20.0, min_width_pct=1.5, max_width_pct=8.0, min_buffer_pct=0.5, max_buffer_pct=4.0,
    atr_multiplier=1.5, min_long_score=0.2)
_GL_INT_PARAMS = ("n",)
_GL_FLAGS = (torch.uint8, torch.bool)
_GL_SYM = (("ok", _GL_FLAGS), ("micro_regime", (torch.uint8,)), ("micro_transition", (torch.uint8,)),
           ("above_ema20", _GL_FLAGS), ("above_ema50", _GL_FLAGS), ("rs_vs_btc", (torch.float64,)),
           ("atr_pct", (torch.float64,)))


@device_entry
def grid_ladder_replay(c: torch.Tensor, bb_upper: torch.Tensor, bb_mid: torch.Tensor, bb_lower: torch.Tensor,
                       market_regime: torch.Tensor, long_regime_score: torch.Tensor,
                       ctx_ok: torch.Tensor | None = None, policy_ok: torch.Tensor | None = None, *, bands=None,
                       sym=None, first_t=None, lens=None, from_t=None, columns=_lib.GL_VALUES, **params):
    """LadderDeployer.signal() replayed over the panel
    (strategies/grid/ladder_deployer.py:58-187; bq_grid_ladder_replay): column
    t of row s = the method on the message whose frame is
    df_15m.iloc[first_t[s]:t + 1] with current_price = close[t]; candles
    max(from_t[s], first_t[s]) .. lens[s] - 1 are replayed. ENABLED and the
    futures check are the caller's; the method keeps no state. c and the
    frame's bb_upper / bb_mid / bb_lower (what _bb_stable iterates over) [S, T]
    float64 with unit stride along T and any row pitch. bands: None (the
    frame's columns are what signal() receives; each is read once) or the
    (bb_high, bb_mid, bb_low) [S, T] float64 tensors as the caller rounded
    them. Per candle time, on the device, [1] (one message) or [T]:
    market_regime int8 (_lib.MARKET_REGIMES codes, negative: None),
    long_regime_score float64, ctx_ok bool / uint8 (False: latest_market_context
    is None; None: present), policy_ok bool / uint8
    (grid_only_policy.allow_grid_ladder; None: allowed). sym: None (no symbol
    has features in the snapshot) or the (ok uint8 / bool, micro_regime uint8,
    micro_transition uint8, above_ema20, above_ema50 uint8 / bool, rs_vs_btc
    float64, atr_pct float64) tensors, all [S] or all [S, T]; the codes index
    _lib.MICRO_REGIMES / _lib.MICRO_TRANSITIONS, _lib.MR_NONE for None. Returns
    (status uint8 [S, T] (_lib.GL_REASONS' indices), {name: float64 [S, T]}
    for `columns`, a subset of _lib.GL_VALUES, NaN where the method did not
    compute them). Nothing is read back and every allocation is by shape: the
    call can be captured. params: GRID_LADDER_DEFAULTS' keys."""
    par = _replay_params("grid_ladder_replay", GRID_LADDER_DEFAULTS, params, _GL_INT_PARAMS)
    if not 1 <= int(par["n"]) <= _lib.BB_STABLE_MAX_N:
        raise ValueError(f"grid_ladder_replay: n in 1..{_lib.BB_STABLE_MAX_N}")
    columns = tuple(columns)
    _replay_columns("grid_ladder_replay", columns, _lib.GL_VALUES)
    S, T = _replay_shape(c)
    bb = [(bb_upper, "bb_upper"), (bb_mid, "bb_mid"), (bb_lower, "bb_lower")]
    if bands is not None and len(bands) != 3:
        raise ValueError("bands: expected (bb_high, bb_mid, bb_low)")
    bd = list(zip(bands, ("bb_high", "bb_mid_arg", "bb_low"))) if bands is not None else []
    _replay_panels([(c, "close")] + bb + bd, S, T)
    mk = _replay_regime(market_regime, "market_regime", ((1,), (T,)))
    if mk is None:
        raise ValueError("market_regime: expected an int8 tensor of shape (1,) or (T,) (negative codes: None)")
    Tc = int(mk.numel())
    if (not isinstance(long_regime_score, torch.Tensor) or long_regime_score.dtype != torch.float64
            or tuple(long_regime_score.shape) != (Tc,)):
        raise ValueError(f"long_regime_score: expected a float64 tensor of shape {(Tc,)}")
    for x, name in ((ctx_ok, "ctx_ok"), (policy_ok, "policy_ok")):
        if x is not None and (not isinstance(x, torch.Tensor) or x.dtype not in _GL_FLAGS or tuple(x.shape) != (Tc,)):
            raise ValueError(f"{name}: expected a bool / uint8 tensor of shape {(Tc,)}")
    sy, ld_sym = _replay_sym(sym, _GL_SYM, S, T)
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S)
    cc = _check_panel(c, "close")
    bbs, ld_bb = _common_pitch([_check_panel(x, n) for x, n in bb])
    bds, ld_bd = _common_pitch([_check_panel(x, n) for x, n in bd]) if bd else ([None] * 3, ld_bb)
    _replay_on_device("market_regime / long_regime_score / ctx_ok / policy_ok / sym",
                      [mk, long_regime_score, ctx_ok, policy_ok, *sy])
    mk, sc = mk.contiguous(), long_regime_score.contiguous()
    cok = ctx_ok.contiguous() if ctx_ok is not None else None
    pok = policy_ok.contiguous() if policy_ok is not None else None
    dev = c.device
    lens, first_t, from_t = _replay_rows(lens, first_t, from_t, S, dev)
    p = _replay_struct(_lib.BqGridLadderParams, par, _GL_INT_PARAMS)
    status, outs, vals = _replay_outputs(columns, _lib.GL_VALUES, S, T, dev)
    st = _lib.load().bq_grid_ladder_replay(
        _ptr(cc), _row_stride(cc), _ptr(bbs[0]), _ptr(bbs[1]), _ptr(bbs[2]), ld_bb, _ptr(bds[0]), _ptr(bds[1]),
        _ptr(bds[2]), ld_bd, _ptr(pok), _ptr(cok), _ptr(mk), _ptr(sc), Tc, _ptr(sy[0]), _ptr(sy[1]), _ptr(sy[2]),
        _ptr(sy[3]), _ptr(sy[4]), _ptr(sy[5]), _ptr(sy[6]), ld_sym, _ptr(lens), _ptr(first_t), _ptr(from_t), S, T,
        ctypes.byref(p), _ptr(status), vals, T, _stream_handle(None))
    _lib.check(st, "bq_grid_ladder_replay")
    return status, outs


def _join_capacity(ts: torch.Tensor, lens: torch.Tensor | None, bts: torch.Tensor) -> int:
    """Largest per-row count of (candle, benchmark row) matches over the
    candles t >= 1 that join (bench_ts ascending): an upper bound on every
    row's joined pairs (dropna only removes some)."""
    S, T = ts.shape
    if S == 0 or T < 2 or bts.numel() == 0:
        return T
    # a benchmark without repeated times joins each candle at most once: T
    # (one small reduction over the benchmark, not a search per candle)
    if bts.numel() < 2 or not bool((bts[1:] == bts[:-1]).any()):
        return T
    keys = ts[:, 1:].contiguous()
    mult = torch.searchsorted(bts, keys, right=True) - torch.searchsorted(bts, keys)
    if lens is not None:
        live = torch.arange(1, T, device=ts.device)[None, :] < lens.reshape(-1, 1)
        mult = torch.where(live, mult, torch.zeros_like(mult))
    return int(mult.sum(dim=1).max().item())


@device_entry
def join_returns(ts: torch.Tensor, close: torch.Tensor, bench_ts: torch.Tensor, bench_close: torch.Tensor,
                 lens=None, capacity: int | None = None, stream: torch.cuda.Stream | None = None):
    """Aligned (symbol, benchmark) log-return pairs of
    ContextEvaluator.dynamic_btc_beta_corr (producers/context_evaluator.py:161-177):
    returns on each frame's own rows, inner join on the timestamp, dropna,
    compacted per row. Returns (x [S, C], y [S, C], pairs per row int64 [S]).
    A benchmark time held k times joins k pairs (pandas' inner join; a frame
    repeating its own time k_l times joins k_l * k times), so a row can hold
    more than T pairs. capacity=None: C = the largest row's joined-row count
    (each candle's benchmark multiplicity, summed per row, on the device: one
    host synchronisation), so no row is ever cut. An int capacity (fixed
    geometry, e.g. a captured graph) gives C = max(T, capacity) without the
    synchronisation; a row with more pairs than C is then cut at C, keeping
    its oldest pairs — size it from the benchmark's repeats. capacity=None
    cannot be used under hipGraph capture (it reads the repeat check back to
    the host): a capturing caller gets a ValueError asking for capacity."""
    ts = _check_ts(ts)
    S, T = ts.shape
    close = _check_panel(close, "close", (S, T)).contiguous()
    bts = _check_ts(bench_ts, "bench_ts").reshape(-1)
    bc = _check_panel(bench_close.reshape(1, -1), "bench_close", (1, bts.numel())).contiguous()
    lens = _check_lens(lens, S, ts.device)
    if capacity is None:
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("join_returns: capacity=None synchronises with the host and cannot run under "
                             "graph capture; pass capacity= (e.g. T when the benchmark repeats no time)")
        capacity = _join_capacity(ts, lens, bts)
    C = max(T, int(capacity))
    x = torch.empty((S, C), dtype=torch.float64, device=ts.device)
    y = torch.empty_like(x)
    n = torch.empty(S, dtype=torch.int64, device=ts.device)
    st = _lib.load().bq_join_returns(_ptr(ts), _ptr(close), _ptr(lens), S, T, T, _ptr(bts), _ptr(bc), bts.numel(),
                                     _ptr(x), _ptr(y), C, _ptr(n), _stream_handle(stream))
    _lib.check(st, "bq_join_returns")
    return x, y, n


@device_entry
def beta_corr_pairs(x: torch.Tensor, y: torch.Tensor, window: int = 50,
                    stream: torch.cuda.Stream | None = None) -> dict[str, torch.Tensor]:
    """Rolling beta / corr over aligned return pairs (join_returns output):
    NaN for rows < window - 1."""
    x = _check_panel(x, "x").contiguous()
    S, T = x.shape
    y = _check_panel(y, "y", (S, T)).contiguous()
    beta = torch.empty((S, T), dtype=torch.float64, device=x.device)
    corr = torch.empty_like(beta)
    st = _lib.load().bq_beta_corr_pairs(_ptr(x), _ptr(y), S, T, T, int(window), _ptr(beta), _ptr(corr), T,
                                        _stream_handle(stream))
    _lib.check(st, "bq_beta_corr_pairs")
    return {"beta": beta, "corr": corr}


@device_entry
def pct_change(x: torch.Tensor, periods: int = 1, fill_method: str | None = "pad") -> torch.Tensor:
    """x.pct_change(periods) along T of a [S, T] panel with pandas 2.3.3's
    default fill_method='pad': f / f.shift(periods) - 1 over the
    forward-filled series f (leading NaNs stay NaN; [1, 2, nan, 4, 5] ->
    [nan, 1, 0, 1, 0.25]) — the BTC 24h change of
    producers/context_evaluator.py:427-430. fill_method=None: the raw series.
    The fill is the device ffill replay (bq_rolling_batch), the quotient the
    same IEEE operations as pandas."""
    x = _check_panel(x, "x")
    if fill_method not in ("pad", "ffill", None):
        raise ValueError(f"fill_method must be 'pad' or None, got {fill_method!r}")
    periods = int(periods)
    if periods < 1:
        raise ValueError(f"periods must be >= 1, got {periods}")
    f = rolling_many(Ffill(x))[0] if fill_method is not None else x
    out = torch.full_like(f, float("nan"))
    if periods < f.shape[1]:
        out[:, periods:] = f[:, periods:] / f[:, :-periods] - 1
    return out