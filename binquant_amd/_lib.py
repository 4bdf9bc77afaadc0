"""ctypes binding of the gfx950 HIP library (``include/binquant_amd.h``).

The library is built in-tree by ``make`` (or ``__graft_entry__.build()``) into
``binquant_amd/lib/libbinquant_amd.so``. There is no CPU fallback: if the
library is missing, or a call returns a non-zero status, this module raises.

torch is imported first so that the HIP runtime torch ships
(``libamdhip64.so.7``) is the one the loader binds our library to; device
pointers and streams are then shared with torch's allocator and streams.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch  # noqa: F401  (binds libamdhip64.so.7 before our library loads)

LIB_PATH = Path(os.environ.get("BQ_LIB_PATH", Path(__file__).resolve().parent / "lib" / "libbinquant_amd.so"))

BQ_OK = 0
BQ_EINVAL = -1
BQ_EHIP = -2
BQ_ESTATE = -4

ENRICH_COLUMNS = (
    "ma_7",
    "ma_25",
    "ma_100",
    "macd",
    "macd_signal",
    "rsi",
    "bb_upper",
    "bb_mid",
    "bb_lower",
    "ATR",
    "twap",
    "ema20",
    "ema50",
    "mfi",
)
INPUT_FIELDS = ("open", "high", "low", "close", "volume")
FEATURE_COLUMNS = ("return_pct", "ema20", "ema50", "trend_score", "atr_pct", "bb_width")
PARTIAL_COLUMNS = (
    "count",
    "advancers",
    "decliners",
    "above_ema20",
    "above_ema50",
    "sum_return",
    "sum_trend",
    "sum_atr_pct",
    "sum_bb_width",
    "tracked",   # 0 from the kernel; market_regime.batch.reduce_partials folds the shard's symbol count in
                 # (bq_breadth_partial_fresh writes the shard's per-timestamp tracked count itself)
)
MAX_WINDOW = 126
MAX_RESAMPLE_FIELDS = 12
STORE_MAX_BARS = 512
MICRO_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "VOLATILE", "TRANSITIONAL")
MICRO_TRANSITIONS = ("VOLATILITY_EXPANSION", "BREAKOUT_UP", "BREAKDOWN", "RECOVERY", "MEAN_REVERSION",
                     "ENTERED_TREND_UP", "ENTERED_TREND_DOWN", "ENTERED_RANGE", "ENTERED_TRANSITIONAL")
# bq_symbol_regime_panel's output columns, the order of bq_regime_panel_u8 / bq_regime_panel_f64
REGIME_PANEL_U8 = ("ok", "micro_regime", "micro_transition", "above_ema20", "above_ema50")
REGIME_PANEL_F64 = ("rs_vs_btc", "micro_regime_strength", "micro_transition_strength", "trend_score", "atr_pct",
                    "bb_width")
REGIME_PANEL_COLUMNS = REGIME_PANEL_U8 + REGIME_PANEL_F64
SCORE_FIELDS = ("confidence", "breadth_score", "btc_alignment_score", "cross_asset_confirmation",
                "followthrough_score", "adverse_excursion_risk", "override_strength", "supportiveness_score",
                "adjusted_score")
AGG_CODES = {"first": 0, "last": 1, "max": 2, "min": 3, "sum": 4}
MAX_ROLLING_WINDOW = 96
ROLL_MODES = {"quantile": 0, "median": 1, "mean": 2, "sum": 3, "var": 4, "std": 5, "var0": 6, "std0": 7,
              "isum": 10,   # isum: sum of an integer-valued series (flag counts), bq_roll_mode BQ_ROLL_ISUM
              "qlower": 11}   # quantile(q, interpolation="lower"), BQ_ROLL_QLOWER
ROLL_EWM = 8
ROLL_FFILL = 9
ROLL_ISUM = 10
MAX_ROLL_JOBS = 16


class BqParams(ctypes.Structure):
    """Mirror of ``bq_params`` (include/binquant_amd.h)."""

    _fields_ = [
        ("ma_periods", ctypes.c_int32 * 3),
        ("macd_fast", ctypes.c_int32),
        ("macd_slow", ctypes.c_int32),
        ("macd_signal", ctypes.c_int32),
        ("rsi_window", ctypes.c_int32),
        ("bb_window", ctypes.c_int32),
        ("bb_ddof", ctypes.c_int32),
        ("atr_window", ctypes.c_int32),
        ("twap_window", ctypes.c_int32),
        ("ema_spans", ctypes.c_int32 * 2),
        ("mfi_window", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("bb_k", ctypes.c_double),
    ]


class BqStoreView(ctypes.Structure):
    """Mirror of ``bq_store_view`` (include/binquant_amd.h)."""

    _fields_ = [
        ("ts", ctypes.c_void_p),
        ("field", ctypes.c_void_p * 5),
        ("head", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("last", ctypes.c_void_p),
        ("capacity", ctypes.c_int64),
        ("max_bars", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


FUSED_MAX_INS = 192
FUSED_MAX_CONST = 32
FUSED_MAX_IN = 16
FUSED_MAX_OUT = 24
FUSED_MAX_REGS = 20
FUSED_MAX_LOADS = 16
FUSED_F64, FUSED_U8 = 0, 1
FUSED_OPS = {name: i for i, name in enumerate(
    ["LD", "CONST", "INRANGE", "ADD", "SUB", "MUL", "DIV", "FMAX", "FMIN", "MAXIMUM", "MINIMUM", "GT", "GE", "LT",
     "LE", "EQ", "NE", "AND", "OR", "NOT", "ABS", "NEG", "ISNAN", "SQRT", "LOG", "WHERE", "ST"], start=1)}


class BqFusedOperand(ctypes.Structure):
    """Mirror of ``bq_fused_operand``."""

    _fields_ = [("ptr", ctypes.c_void_p), ("stride_s", ctypes.c_int64), ("stride_t", ctypes.c_int64),
                ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BqFusedProgram(ctypes.Structure):
    """Mirror of ``bq_fused_program``."""

    _fields_ = [
        ("n_ins", ctypes.c_int32), ("n_loads", ctypes.c_int32), ("n_regs", ctypes.c_int32),
        ("n_in", ctypes.c_int32), ("n_out", ctypes.c_int32), ("n_const", ctypes.c_int32),
        ("ins", ctypes.c_uint64 * FUSED_MAX_INS),
        ("consts", ctypes.c_double * FUSED_MAX_CONST),
        ("inp", BqFusedOperand * FUSED_MAX_IN),
        ("out", BqFusedOperand * FUSED_MAX_OUT),
    ]


class BqRollJob(ctypes.Structure):
    """Mirror of ``bq_roll_job`` (include/binquant_amd.h)."""

    _fields_ = [
        ("x", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("ld_in", ctypes.c_int64),
        ("ld_out", ctypes.c_int64),
        ("window", ctypes.c_int32),
        ("min_periods", ctypes.c_int32),
        ("shift", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("q", ctypes.c_double),
        ("alpha", ctypes.c_double),
        ("rows", ctypes.c_int64),
        ("panel", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class BqContextScalars(ctypes.Structure):
    _fields_ = [("confidence", ctypes.c_double), ("long_tailwind", ctypes.c_double),
                ("short_tailwind", ctypes.c_double), ("btc_regime_score", ctypes.c_double),
                ("market_stress_score", ctypes.c_double), ("present", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BqScorerWeights(ctypes.Structure):
    _fields_ = [("context_weight", ctypes.c_double), ("risk_weight", ctypes.c_double),
                ("support_weight", ctypes.c_double)]


class BqImpulseParams(ctypes.Structure):
    """Mirror of ``bq_impulse_params`` (include/binquant_amd.h)."""

    _fields_ = [("min_impulse", ctypes.c_double), ("max_impulse", ctypes.c_double), ("min_rs", ctypes.c_double),
                ("max_btc_return", ctypes.c_double), ("min_conf_return", ctypes.c_double),
                ("min_close_location", ctypes.c_double), ("max_atr_pct", ctypes.c_double),
                ("entry_factor", ctypes.c_double), ("min_history", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# bq_impulse_rider: status codes (BQ_IR_*), value-column order, tile size
IMPULSE_TILE = 1024
BB_STABLE_MAX_N = 64
(BQ_IR_CONFIRMED, BQ_IR_SHORT_HISTORY, BQ_IR_INVALID_VALUES, BQ_IR_INVALID_ANCHORS, BQ_IR_BTC_UNAVAILABLE,
 BQ_IR_RANGE_INVALID, BQ_IR_NOT_READY, BQ_IR_IMPULSE_RANGE, BQ_IR_DID_NOT_CROSS, BQ_IR_BTC_TOO_HIGH,
 BQ_IR_RS_TOO_LOW, BQ_IR_ATR_TOO_HIGH, BQ_IR_DID_NOT_HOLD, BQ_IR_CONFIRMATION_NEGATIVE,
 BQ_IR_CLOSE_NOT_NEAR_HIGH) = range(15)
BQ_IR_NO_FRAME = 255
IMPULSE_VALUES = ("impulse_return_1h", "previous_impulse_return_1h", "btc_return_1h", "relative_strength_1h",
                  "trigger_return_15m", "confirmation_return_15m", "confirmation_close_location", "atr_pct",
                  "entry_limit_price")


class BqRetestParams(ctypes.Structure):
    """Mirror of ``bq_retest_params`` (include/binquant_amd.h)."""

    _fields_ = [("watch_ms", ctypes.c_int64), ("min_history", ctypes.c_int32), ("breakout_lookback", ctypes.c_int32),
                ("support_factor", ctypes.c_double), ("pullback_factor", ctypes.c_double)]


# bq_retest_replay: event codes (BQ_RT_*), detail bits (BQ_RT_D_*)
RETEST_MAX_LOOKBACK = 64
(BQ_RT_IDLE, BQ_RT_WATCH_SET, BQ_RT_WATCHING, BQ_RT_RISK_BLOCKED, BQ_RT_CANDIDATE, BQ_RT_SHORT_HISTORY) = range(6)
BQ_RT_NO_FRAME = 255
BQ_RT_D_SUPPORT, BQ_RT_D_PULLBACK, BQ_RT_D_RECLAIM, BQ_RT_D_EXPIRED = 1, 2, 4, 8
RT_EVENTS = ("idle", "watch_set", "watching", "risk_blocked", "candidate", "history_too_short")


class BqSpikeFadeParams(ctypes.Structure):
    """Mirror of ``bq_spike_fade_params`` (include/binquant_amd.h)."""

    _fields_ = [("window_bars", ctypes.c_int32), ("ext_factor", ctypes.c_double)]


class BqSpikeFramesParams(ctypes.Structure):
    """Mirror of ``bq_spike_frames_params`` (include/binquant_amd.h)."""

    _fields_ = [("volume_cluster_window", ctypes.c_int32), ("volume_cluster_min_count", ctypes.c_int32),
                ("cumulative_price_window", ctypes.c_int32), ("label_mode", ctypes.c_int32),
                ("require_both_patterns", ctypes.c_int32), ("require_bullish_spike", ctypes.c_int32),
                ("post_spike_cooldown_bars", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("cumulative_price_threshold", ctypes.c_double), ("body_size_pct_min", ctypes.c_double),
                ("volume_cluster_min_ratio", ctypes.c_double), ("price_break_base_threshold", ctypes.c_double),
                ("volume_quantile", ctypes.c_double), ("price_base_floor_quantile", ctypes.c_double),
                ("min_volume_ratio", ctypes.c_double), ("min_price_abs_floor", ctypes.c_double)]


# bq_spike_frames: the caps (BQ_SPIKE_FRAMES_MAX_*), the input columns (enum bq_spike_frames_in / _in_b) and the
# byte outputs (enum bq_spike_frames_out) under their detect() / latest_signal() names
SPIKE_FRAMES_MAX_T = 2048
SPIKE_FRAMES_MAX_WINDOW = 30
SPIKE_FRAMES_MAX_COOLDOWN = 64
SPIKE_FRAMES_IN = ("volume_ratio", "price_change_abs", "dyn_threshold", "body_size_pct", "cum_pos", "cum_neg", "open",
                   "close")
SPIKE_FRAMES_IN_B = ("accel_spike_flag", "accel_spike_short_flag", "upward", "downward")
SPIKE_FRAMES_OUT = ("label", "label_pre", "label_short", "label_short_pre", "volume_cluster_flag", "price_break_flag",
                    "cumulative_price_break_flag", "cumulative_price_break_short_flag", "accel_spike_flag",
                    "accel_spike_short_flag", "upward", "downward")
# bq_spike_frames_capped: the smallest frame_cap (BQ_SPIKE_FRAMES_MIN_CAP; the largest is SPIKE_FRAMES_MAX_T) and the
# int32 columns (enum bq_spike_frames_in_i)
SPIKE_FRAMES_MIN_CAP = 64
SPIKE_FRAMES_IN_I = ("dyn_src", "close_next")


class BqSpikeFramesCap(ctypes.Structure):
    """Mirror of ``bq_spike_frames_cap`` (include/binquant_amd.h)."""

    _fields_ = [("frame_cap", ctypes.c_int32), ("base_window", ctypes.c_int32),
                ("accel_volume_deriv_window", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("price_break_dynamic_q", ctypes.c_double)]


# bq_spike_fade_replay: event codes (BQ_FS_*), detail bits (BQ_FS_D_*)
SPIKEFADE_MAX_WINDOW = 32
(BQ_FS_IDLE, BQ_FS_SOURCE_SET, BQ_FS_WAITING, BQ_FS_CANDIDATE, BQ_FS_CLEARED, BQ_FS_SAME_CANDLE) = range(6)
BQ_FS_NO_FRAME = 255
(BQ_FS_D_SOURCE, BQ_FS_D_MARKET, BQ_FS_D_NEW_HIGH, BQ_FS_D_CANDLE_EXPIRED, BQ_FS_D_WINDOW_EXPIRED,
 BQ_FS_D_EXTENSION) = 1, 2, 4, 8, 16, 32
FS_EVENTS = ("idle", "source_set", "waiting", "candidate", "cleared", "same_candle")


class BqPriceTrackerParams(ctypes.Structure):
    """Mirror of ``bq_price_tracker_params`` (include/binquant_amd.h)."""

    _fields_ = [("min_history", ctypes.c_int32), ("tail_rows", ctypes.c_int32), ("span_fast", ctypes.c_int32),
                ("span_slow", ctypes.c_int32), ("rsi_max", ctypes.c_double), ("macd_max", ctypes.c_double),
                ("mfi_max", ctypes.c_double), ("w_rsi", ctypes.c_double), ("w_mfi", ctypes.c_double),
                ("w_macd", ctypes.c_double), ("macd_scale", ctypes.c_double), ("context_weight", ctypes.c_double),
                ("risk_weight", ctypes.c_double), ("support_weight", ctypes.c_double),
                ("min_followthrough", ctypes.c_double), ("max_risk", ctypes.c_double),
                ("min_confidence", ctypes.c_double), ("cooldown_ms", ctypes.c_int64)]


# bq_price_tracker_replay: status codes (BQ_PT_*, the index is the code; the reference returns silently, so the
# names are this library's), detail bits (BQ_PT_D_*), the value columns' order, the context rows' order
PT_MAX_TAIL_ROWS = 64
(BQ_PT_EMIT, BQ_PT_NO_FRAME, BQ_PT_NOT_READY, BQ_PT_NO_SETUP, BQ_PT_NO_CONTEXT, BQ_PT_CONTEXT_REJECTED,
 BQ_PT_COOLDOWN) = range(7)
BQ_PT_D_FOLLOWTHROUGH, BQ_PT_D_RISK, BQ_PT_D_CONFIDENCE = 1, 2, 4
PT_REASONS = ("emit", "no_frame", "not_enough_data", "not_oversold", "market_context_unavailable",
              "context_rejected", "entry_cooldown_active")
PT_DETAILS = {BQ_PT_D_FOLLOWTHROUGH: "bad_followthrough", BQ_PT_D_RISK: "high_risk",
              BQ_PT_D_CONFIDENCE: "low_confidence"}
PT_VALUES = ("local_score", "trend_score", "followthrough", "adverse_risk", "supportiveness", "adjusted_score")
PT_CTX_ROWS = ("confidence", "long_tailwind", "btc_regime_score", "market_stress_score")
# LiveMarketContext.market_regime's literals (market_regime/models.py:7-13), the index is the code
MARKET_REGIMES = ("TREND_UP", "TREND_DOWN", "RANGE", "HIGH_STRESS", "TRANSITIONAL")


class BqMeanReversionParams(ctypes.Structure):
    """Mirror of ``bq_mean_reversion_params`` (include/binquant_amd.h)."""

    _fields_ = [("rsi_window", ctypes.c_int32), ("volume_ma_window", ctypes.c_int32), ("atr_ma_window", ctypes.c_int32),
                ("ema_fast", ctypes.c_int32), ("ema_slow", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rsi_short_min", ctypes.c_double), ("volume_ratio_min", ctypes.c_double),
                ("atr_spike_max", ctypes.c_double), ("atr_stop_mult", ctypes.c_double),
                ("max_entry_stop_loss_pct", ctypes.c_double), ("max_trend_score", ctypes.c_double),
                ("max_market_stress", ctypes.c_double), ("max_gap", ctypes.c_double),
                ("max_symbol_atr_pct", ctypes.c_double), ("min_wick_ratio", ctypes.c_double)]


# bq_mean_reversion_replay: status codes (BQ_MR_*, the index is the code; 2-16 are the reference's own log reasons),
# the value columns' order (the first MR_NFEATURES are the optional given features), the context rows' order, the
# code of a None micro_regime / micro_regime_transition (the others: indices into MICRO_REGIMES / MICRO_TRANSITIONS)
MR_MAX_WINDOW = 64
MR_REASONS = ("emit", "no_frame", "indicators_not_ready", "atr_volatility_spike", "volume_below_average",
              "invalid_candle_range", "no_fade_setup", "trend_score_above_max", "market_context_unavailable",
              "market_stress_too_high", "symbol_atr_too_high", "market_context_long_edge", "btc_context_up",
              "symbol_breakout_up", "symbol_trend_up", "candle_already_emitted", "entry_stop_loss_too_wide")
MR_VALUES = ("rsi", "previous_rsi", "volume_ma", "atr_ma", "trend_score", "stop_loss_pct", "score")
MR_NFEATURES = 5
MR_CTX_ROWS = ("market_stress_score", "long_regime_score", "short_regime_score", "btc_regime_score", "btc_return")
MR_NONE = 255


class BqRangeFadeParams(ctypes.Structure):
    """Mirror of ``bq_range_fade_params`` (include/binquant_amd.h)."""

    _fields_ = [("min_candles", ctypes.c_int32), ("adx_window", ctypes.c_int32), ("zscore_window", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("adx_max", ctypes.c_double), ("long_rsi_max", ctypes.c_double),
                ("short_rsi_min", ctypes.c_double), ("long_zscore_max", ctypes.c_double),
                ("short_zscore_min", ctypes.c_double), ("band_touch_tolerance", ctypes.c_double),
                ("max_market_stress", ctypes.c_double), ("max_symbol_atr_pct", ctypes.c_double),
                ("max_symbol_bb_width", ctypes.c_double), ("min_rejection_wick_frac", ctypes.c_double),
                ("long_close_position_min", ctypes.c_double), ("short_close_position_max", ctypes.c_double)]


# bq_range_fade_replay: status codes (BQ_RF_*, the index is the code; 2-14 are the points where
# RangeBbRsiMeanReversion.signal() returns, regime_routing's reasons by their fixed part), the value columns' order
# (the first RF_NFEATURES are the optional given features), the context rows' order (market_regime: an index into
# MARKET_REGIMES, MR_NONE for None), the windows' limits
RF_MAX_ADX_WINDOW, RF_MAX_ZSCORE_WINDOW = 32, 64
RF_REASONS = ("emit", "no_frame", "not_enough_data", "market_context_unavailable", "market_transitioning",
              "market_stress_too_high", "market_regime_unavailable", "market_regime_not_range",
              "symbol_regime_unavailable", "symbol_regime_not_range", "symbol_transition", "symbol_atr_too_high",
              "symbol_bb_width_too_high", "adx_too_high", "no_bb_rsi_rejection_setup")
RF_VALUES = ("adx", "zscore", "direction", "score")
RF_NFEATURES = 2
RF_CTX_ROWS = ("regime_is_transitioning", "market_stress_score", "market_regime")


class BqBuyTheDipParams(ctypes.Structure):
    """Mirror of ``bq_buy_the_dip_params`` (include/binquant_amd.h)."""

    _fields_ = [("lookback_candles", ctypes.c_int32), ("ema_span", ctypes.c_int32), ("lookback_ms", ctypes.c_int64),
                ("start_time_ms", ctypes.c_int64), ("min_change_pct", ctypes.c_double),
                ("max_change_pct", ctypes.c_double)]


# bq_buy_the_dip_replay: status codes (BQ_DIP_*, the index is the code: the points where BuyTheDip.signal() returns,
# in its order; the reference returns silently or with a log line, so the names are this library's) and the value
# columns' order. market_regime / micro_regime: int8 indices into MARKET_REGIMES / MICRO_REGIMES, negative for None
(BQ_DIP_EMIT, BQ_DIP_NO_FRAME, BQ_DIP_NOT_READY, BQ_DIP_BEFORE_START, BQ_DIP_NO_REFERENCE, BQ_DIP_OUT_OF_BAND,
 BQ_DIP_REGIME_BLOCKED, BQ_DIP_NOT_RECLAIMED) = range(8)
DIP_REASONS = ("emit", "no_frame", "not_enough_data", "before_start_time", "no_reference_price",
               "change_outside_dip_band", "blocked_trend_regime", "prior_close_and_ema20_not_reclaimed")
DIP_VALUES = ("reference_price", "change_6h", "ema20")


class BqBbExtremeParams(ctypes.Structure):
    """Mirror of ``bq_bb_extreme_params`` (include/binquant_amd.h)."""

    _fields_ = [("lookback", ctypes.c_int32), ("rsi_window", ctypes.c_int32), ("oversold_rsi", ctypes.c_double),
                ("overbought_rsi", ctypes.c_double), ("max_lower_band_position", ctypes.c_double),
                ("min_upper_band_position", ctypes.c_double)]


# bq_bb_extreme_replay: status codes (BQ_BBX_*, the index is the code: the points where BBExtremeReversion.signal()
# returns, in its order; the names restate its log lines and evaluate()'s reasons) and the value columns' order.
# direction: bq_direction as a double (0.0 LONG = buy, 1.0 SHORT = sell)
(BQ_BBX_EMIT, BQ_BBX_NO_FRAME, BQ_BBX_NOT_ENOUGH_DATA, BQ_BBX_NULLS, BQ_BBX_NO_RSI, BQ_BBX_INVALID_BAND,
 BQ_BBX_NO_EXTREME) = range(7)
BBX_REASONS = ("emit", "no_frame", "not_enough_data", "recent_data_contains_nulls", "not_enough_candles_for_rsi",
               "invalid_band_spread", "no_extreme")
BBX_VALUES = ("rsi_value", "band_position", "bb_width", "distance_from_mid_pct", "direction")
BBX_MAX_LOOKBACK = 64


class BqRsReversalParams(ctypes.Structure):
    """Mirror of ``bq_rs_reversal_params`` (include/binquant_amd.h)."""

    _fields_ = [("window", ctypes.c_int32), ("reserved", ctypes.c_int32), ("quantile", ctypes.c_double),
                ("avg_return_max", ctypes.c_double), ("rs_min", ctypes.c_double)]


# bq_rs_reversal_replay: status codes (BQ_RSR_*, the index is the code: the points where
# RelativeStrengthReversalRange.signal() returns, in its order; 3, 4, 6, 7, 8 are regime_routing's own reasons, 5 its
# "market_regime_<name>" by the fixed part; the others are this library's names) and the value columns' order.
# market_regime: int8 indices into MARKET_REGIMES, negative for None
(BQ_RSR_EMIT, BQ_RSR_NO_FRAME, BQ_RSR_SHORT_FRAME, BQ_RSR_NO_CONTEXT, BQ_RSR_REGIME_NONE, BQ_RSR_NOT_RANGE,
 BQ_RSR_MARKET_NOT_WEAK, BQ_RSR_NO_FEATURES, BQ_RSR_RS_INSUFFICIENT, BQ_RSR_DEAD_TAPE) = range(10)
RSR_REASONS = ("emit", "no_frame", "short_frame", "market_context_unavailable",
               "market_regime_unavailable", "market_regime_not_range", "market_avg_return_not_weak_enough",
               "symbol_regime_unavailable", "symbol_rs_vs_btc_insufficient", "dead_tape")
RSR_VALUES = ("volume_floor",)
RSR_MAX_WINDOW = 192


class BqGridLadderParams(ctypes.Structure):
    """Mirror of ``bq_grid_ladder_params`` (include/binquant_amd.h)."""

    _fields_ = [("n", ctypes.c_int32), ("reserved", ctypes.c_int32), ("max_change_pct", ctypes.c_double),
                ("min_width_pct", ctypes.c_double), ("max_width_pct", ctypes.c_double),
                ("min_buffer_pct", ctypes.c_double), ("max_buffer_pct", ctypes.c_double),
                ("atr_multiplier", ctypes.c_double), ("min_long_score", ctypes.c_double)]


# bq_grid_ladder_replay: status codes (BQ_GL_*, the index is the code: the points where LadderDeployer.signal()
# returns, in its order, by the fixed part of its "grid_ladder skipped: ..." log line; "emit" and "no_frame" are this
# library's), the value columns' order, the context rows' order of signals.grid_ladder_entry (market_regime: an index
# into MARKET_REGIMES, negative for None; micro_regime / micro_transition: MR_NONE for None) and the tile width
(BQ_GL_EMIT, BQ_GL_NO_FRAME, BQ_GL_POLICY, BQ_GL_NO_CONTEXT, BQ_GL_NOT_RANGE, BQ_GL_MICRO_REGIME,
 BQ_GL_SYMBOL_TRANSITION, BQ_GL_BELOW_EMAS, BQ_GL_RS_NOT_POSITIVE, BQ_GL_LONG_SCORE_LOW, BQ_GL_BB_EXPANDING,
 BQ_GL_PRICE_OUTSIDE, BQ_GL_RANGE_WIDTH) = range(13)
GL_REASONS = ("emit", "no_frame", "grid_only_policy", "market_context_unavailable", "market_regime_not_range",
              "symbol_micro_regime", "symbol_transition", "symbol_below_ema20_and_ema50",
              "relative_strength_vs_btc_not_positive", "long_regime_score_too_low", "bb_width_expanding",
              "price_outside_range", "range_width")
GL_VALUES = ("bb_change_pct", "range_width_pct", "breakout_buffer_pct", "breakout_low", "breakout_high")
GL_CTX_ROWS = ("market_regime", "long_regime_score")
GRID_LADDER_TILE = 1024


class BqTopGainerParams(ctypes.Structure):
    """Mirror of ``bq_top_gainer_params`` (include/binquant_amd.h)."""

    _fields_ = [("lookback_high", ctypes.c_int32), ("volume_window", ctypes.c_int32), ("min_history", ctypes.c_int32),
                ("full_extension_bars", ctypes.c_int32), ("min_candle_return", ctypes.c_double),
                ("max_candle_return", ctypes.c_double), ("min_return_1h", ctypes.c_double),
                ("min_return_2h", ctypes.c_double), ("min_return_6h", ctypes.c_double),
                ("max_return_1h", ctypes.c_double), ("max_extension", ctypes.c_double),
                ("min_short_extension_cap", ctypes.c_double), ("min_volume_ratio", ctypes.c_double),
                ("min_range_position", ctypes.c_double), ("max_upper_wick", ctypes.c_double),
                ("atr_stop_mult", ctypes.c_double), ("min_stop_loss_pct", ctypes.c_double),
                ("max_stop_loss_pct", ctypes.c_double)]


# bq_top_gainer_entry: entry / status codes (BQ_TGE_*, the index is the code),
# value-column order (_features' key order), the ring's halo
TGE_MAX_LOOKBACK = 96
TGE_REASONS = ("top_gainer_breakout_two_close_confirmation", "history_too_short", "invalid_candle_values",
               "indicators_not_ready", "not_breaking_recent_high", "not_above_ema20_and_ema50",
               "candle_not_green_enough", "single_candle_too_extended", "one_hour_move_too_extended",
               "extension_move_too_extended", "momentum_not_accelerating", "six_hour_move_not_confirmed",
               "volume_ratio_too_low", "close_not_near_high", "upper_wick_too_large",
               "first_confirmation_did_not_hold_breakout", "second_confirmation_did_not_clear_breakout_close",
               "risk_rejected")
TGE_ENTRY_OK = "top_gainer_breakout_ignition"   # code 0 of the `entry` column (status 0: TGE_REASONS[0])
BQ_TGE_CONFIRMED, BQ_TGE_SHORT_HISTORY, BQ_TGE_INVALID_CANDLE, BQ_TGE_NOT_READY = 0, 1, 2, 3
BQ_TGE_FIRST_CONFIRM, BQ_TGE_SECOND_CONFIRM, BQ_TGE_RISK_REJECTED = 15, 16, 17
TGE_NO_FRAME = BQ_TGE_NO_FRAME = 255
TGE_VALUES = ("close", "open", "high", "low", "volume", "quote_volume", "previous_high", "return_1h", "return_2h",
              "return_6h", "extension_return", "extension_window_bars", "extension_cap", "candle_return",
              "volume_ratio", "quote_volume_ratio", "range_position", "upper_wick_fraction", "ema20", "ema50", "atr")


class BqSweepParams(ctypes.Structure):
    """Mirror of ``bq_sweep_params`` (include/binquant_amd.h)."""

    _fields_ = [("min_momentum_atr", ctypes.c_double), ("max_momentum_atr", ctypes.c_double),
                ("min_close_location", ctypes.c_double), ("min_frame", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# bq_sweep_select: the gate columns in _is_candidate's order (:272-286), the status codes (BQ_SW_*, the index is
# the code), the width below which a range runs a lane per row, the wide mapping's tile
SW_COLUMNS = ("pump_score", "score_threshold", "momentum_atr", "close", "prior_high", "close_location",
              "relative_volume", "volume_threshold", "trend_score", "ema20", "relative_strength", "btc_momentum_3",
              "btc_trend_score")
SW_REASONS = ("candidate", "frame_too_short", "required_value_not_finite", "no_score_cross",
              "momentum_atr_out_of_range", "close_not_above_prior_high", "close_location_too_low",
              "relative_volume_below_threshold", "trend_score_not_positive", "close_not_above_ema20",
              "relative_strength_not_positive", "btc_momentum_not_positive", "btc_trend_not_positive",
              "score_threshold_not_positive", "route_refused")
BQ_SW_CANDIDATE, BQ_SW_SHORT_FRAME, BQ_SW_NOT_FINITE, BQ_SW_NO_CROSS = 0, 1, 2, 3
BQ_SW_THRESHOLD_NONPOSITIVE, BQ_SW_ROUTE_REFUSED = 13, 14
SW_NO_FRAME = BQ_SW_NO_FRAME = 255
SW_SWITCH_WIDTH, SW_TILE, SW_ROW_CHUNK = 64, 256, 64

_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_PP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); every symbol declared in include/binquant_amd.h
SIGNATURES: dict[str, tuple] = {
    "bq_default_params": (None, [ctypes.POINTER(BqParams)]),
    "bq_version": (ctypes.c_char_p, []),
    "bq_device_arch": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "bq_enrich": (
        ctypes.c_int,
        [_PP, _I64, _I64, _I64, ctypes.POINTER(BqParams), _PP, _I64, _P],
    ),
    "bq_state_create": (
        ctypes.c_int,
        [ctypes.POINTER(ctypes.c_void_p), _I64, ctypes.POINTER(BqParams)],
    ),
    "bq_state_create_frame": (
        ctypes.c_int,
        [ctypes.POINTER(ctypes.c_void_p), _I64, ctypes.POINTER(BqParams), _I64],
    ),
    "bq_state_destroy": (ctypes.c_int, [_P]),
    "bq_state_seed": (ctypes.c_int, [_P, _PP, _I64, _I64, _P]),
    "bq_tick": (ctypes.c_int, [_P, _PP, _PP, _P]),
    "bq_state_symbols": (_I64, [_P]),
    "bq_state_count": (_I64, [_P]),
    "bq_state_frame": (_I64, [_P]),
    "bq_market_features": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, _PP, _I64, _P]),
    "bq_breadth_partial": (ctypes.c_int, [_P, _PP, _I64, _I64, _I64, _I64, _P, _P]),
    "bq_context_workspace_bytes": (ctypes.c_size_t, [_I64, _I64]),
    "bq_context_partials": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, _P, ctypes.c_size_t, _P, _PP, _P]),
    "bq_panel_compact": (ctypes.c_int, [_PP, _I64, _I64, _I64, _PP, _I64, _P, _I64, _P, _P, _P, _P]),
    "bq_breadth_partial_fresh": (ctypes.c_int, [_P, _PP, _P, _P, _I64, _I64, _I64, _I64, _I64, _P, _P]),
    "bq_pump_ewm": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P]),
    "bq_leadership_workspace_bytes": (ctypes.c_size_t, [_I64, _I64]),
    "bq_leadership": (ctypes.c_int, [_P, _I64, _P, _I64, _I64, _I64, _P, _P, _I64, ctypes.c_double, _I32, _I32, _I32,
                                     _I32, _I32, _P, ctypes.c_size_t, _P, _P, _P, _I64, _P]),
    "bq_impulse_default_params": (None, [ctypes.POINTER(BqImpulseParams)]),
    "bq_impulse_rider": (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _I64, _P, _P, _I64,
                                        ctypes.POINTER(BqImpulseParams), _P, _PP, _I64, _P]),
    "bq_bb_stable": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _I64, _I32, ctypes.c_double, _P, _P, _I64, _P]),
    "bq_grid_ladder_default_params": (None, [ctypes.POINTER(BqGridLadderParams)]),
    "bq_grid_ladder_replay": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _I64,
                                             _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                             ctypes.POINTER(BqGridLadderParams), _P, _PP, _I64, _P]),
    "bq_top_gainer_default_params": (None, [ctypes.POINTER(BqTopGainerParams)]),
    "bq_top_gainer_entry": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _I64,
                                           ctypes.POINTER(BqTopGainerParams), _P, _P, _P, _P, _PP, _I64, _P]),
    "bq_sweep_default_params": (None, [ctypes.POINTER(BqSweepParams)]),
    "bq_sweep_select_workspace": (_I64, [_I64, _I64]),
    "bq_sweep_select": (ctypes.c_int, [_PP, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I64, _I64, _I64,
                                       ctypes.POINTER(BqSweepParams), _P, _P, _I64, _P, _P, _P, _P]),
    "bq_retest_default_params": (None, [ctypes.POINTER(BqRetestParams)]),
    "bq_retest_replay": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                        ctypes.POINTER(BqRetestParams), _P, _P, _P, _P, _P, _P, _I64, _P]),
    "bq_spike_fade_default_params": (None, [ctypes.POINTER(BqSpikeFadeParams)]),
    "bq_spike_fade_replay": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                            ctypes.POINTER(BqSpikeFadeParams), _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "bq_spike_frames_default_params": (None, [ctypes.POINTER(BqSpikeFramesParams)]),
    "bq_spike_frames_workspace": (ctypes.c_size_t, [_I64, _I64]),
    "bq_spike_frames": (ctypes.c_int, [_PP, _I64, _PP, _I64, _I32, _P, _P, _P, _I64, _I64,
                                       ctypes.POINTER(BqSpikeFramesParams), _P, ctypes.c_size_t, _P, _P, _PP, _I64,
                                       _P]),
    "bq_spike_frames_capped_workspace": (ctypes.c_size_t, [_I64, _I64]),
    "bq_spike_frames_capped": (ctypes.c_int, [_PP, _I64, _PP, _I64, _PP, _I64, _I32, _P, _P, _P, _I64, _I64,
                                              ctypes.POINTER(BqSpikeFramesParams), ctypes.POINTER(BqSpikeFramesCap),
                                              _P, ctypes.c_size_t, _P, _P, _PP, _I64, _P]),
    "bq_price_tracker_default_params": (None, [ctypes.POINTER(BqPriceTrackerParams)]),
    "bq_price_tracker_replay": (ctypes.c_int, [_P, _P, _P, _P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64,
                                               _P, _I64, _P, _I64, _P, _P, _P, _I64, _I64,
                                               ctypes.POINTER(BqPriceTrackerParams), _P, _P, _P, _P, _PP, _I64, _P]),
    "bq_mean_reversion_default_params": (None, [ctypes.POINTER(BqMeanReversionParams)]),
    "bq_mean_reversion_replay": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _PP, _I64, _P,
                                                _I64, _P, _I64, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                                ctypes.POINTER(BqMeanReversionParams), _P, _P, _P, _PP, _I64, _P]),
    "bq_range_fade_default_params": (None, [ctypes.POINTER(BqRangeFadeParams)]),
    "bq_range_fade_replay": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _PP, _I64, _P, _I64,
                                            _P, _I64, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                            ctypes.POINTER(BqRangeFadeParams), _P, _PP, _I64, _P]),
    "bq_buy_the_dip_default_params": (None, [ctypes.POINTER(BqBuyTheDipParams)]),
    "bq_buy_the_dip_replay": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I64,
                                             ctypes.POINTER(BqBuyTheDipParams), _P, _PP, _I64, _P]),
    "bq_bb_extreme_default_params": (None, [ctypes.POINTER(BqBbExtremeParams)]),
    "bq_bb_extreme_replay": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                            ctypes.POINTER(BqBbExtremeParams), _P, _PP, _I64, _P]),
    "bq_rs_reversal_default_params": (None, [ctypes.POINTER(BqRsReversalParams)]),
    "bq_rs_reversal_replay": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I64,
                                             ctypes.POINTER(BqRsReversalParams), _P, _PP, _I64, _P]),
    "bq_beta_corr": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I32, _P, _P, _I64, _P]),
    "bq_rolling": (ctypes.c_int, [_P, _I64, _I64, _I64, _I32, _I32, _I32, _I32, ctypes.c_double, _P, _I64, _P]),
    "bq_rolling_quantile_cross": (ctypes.c_int, [_P, _I64, _I64, _I64, _I32, _I32, _I32, ctypes.c_double, _P, _I64,
                                                 _P, _I64, _P]),
    "bq_ewm": (ctypes.c_int, [_P, _I64, _I64, _I64, ctypes.c_double, _I32, _P, _I64, _P]),
    "bq_row_quantile": (ctypes.c_int, [_P, _I64, _I64, _I64, ctypes.c_double, _P, _P]),
    "bq_cooldown": (ctypes.c_int, [_P, _I64, _I64, _I64, _I32, _P, _P, _I64, _P]),
    "bq_pump_features": (ctypes.c_int, [_PP, _I64, _I64, _I64, _PP, _I32, _I32, _I32, _PP, _I64, _P]),
    "bq_pump_features_ewm": (ctypes.c_int, [_PP, _I64, _I64, _I64, _PP, _I32, _I32, _I32, _PP, _I64, _P]),
    "bq_burst_features": (ctypes.c_int, [_PP, _I64, _I64, _I64, _P, _PP, _PP, _P, _I64, _P]),
    "bq_burst_qualify": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _I32, _P, _P]),
    "bq_spike_base": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, _I32, _PP, _PP, _I64, _P]),
    "bq_spike_base_std": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, _I32, _PP, _PP, _PP, _I64, _P]),
    "bq_spike_flags": (ctypes.c_int, [_PP, _P, _P, _I64, _I64, _I64, _P, _PP, _PP, _I64, _P]),
    "bq_supertrend": (ctypes.c_int, [_PP, _I64, _I64, _I64, ctypes.c_double, _P, _P, _P, _I64, _P]),
    "bq_supertrend_hlc": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, ctypes.c_double, _P, _P, _P, _I64, _P]),
    "bq_supertrend_panel": (ctypes.c_int, [_PP, _I64, _I64, _I64, _I32, ctypes.c_double, _P, _P, _P, _I64, _P]),
    "bq_resample_count": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "bq_resample": (ctypes.c_int, [_P, _PP, _P, _I32, _P, _I64, _I64, _I64, _I64, _P, _PP, _I64, _P]),
    "bq_resample_tail": (ctypes.c_int, [_P, _PP, _P, _I32, _P, _I64, _I64, _I64, _I64, _P, _PP, _I64, _P]),
    "bq_align": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P]),
    "bq_join_returns": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _P, _I64, _P, _P]),
    "bq_beta_corr_bret": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I32, _P, _P, _I64, _P]),
    "bq_beta_corr_ws": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I32, _P, _P, _I64, _P]),
    "bq_beta_corr_pairs": (ctypes.c_int, [_P, _P, _I64, _I64, _I64, _I32, _P, _P, _I64, _P]),
    "bq_store_update": (ctypes.c_int, [ctypes.POINTER(BqStoreView), _P, _P, _PP, _P, _I64, _P]),
    "bq_store_features": (ctypes.c_int, [ctypes.POINTER(BqStoreView), _P, _I64, _PP, _P, _P]),
    "bq_store_context_features": (ctypes.c_int, [ctypes.POINTER(BqStoreView), _I64, _P, _I64, _I32, _PP, _P, _P,
                                                 _P, _P]),
    "bq_store_gather": (ctypes.c_int, [ctypes.POINTER(BqStoreView), _P, _I64, _P, _PP, _I64, _P]),
    "bq_rolling_batch": (ctypes.c_int, [ctypes.POINTER(BqRollJob), _I32, _I64, _I64, _P]),
    "bq_rolling_batch_cross": (ctypes.c_int, [ctypes.POINTER(BqRollJob), _I32, _I64, _I64, _PP,
                                              ctypes.POINTER(ctypes.c_int64), _P]),
    "bq_fused_eval": (ctypes.c_int, [ctypes.POINTER(BqFusedProgram), _I64, _I64, _P]),
    "bq_fused_set_native": (ctypes.c_int, [_I32]),
    "bq_fused_set_cache_dir": (ctypes.c_int, [ctypes.c_char_p]),
    "bq_fused_source": (ctypes.c_int, [ctypes.POINTER(BqFusedProgram), ctypes.c_char_p, _I64, ctypes.POINTER(_I64)]),
    "bq_fused_compile": (ctypes.c_int, [ctypes.POINTER(BqFusedProgram)]),
    "bq_fused_stats": (ctypes.c_int, [ctypes.POINTER(_I64)] * 3),
    "bq_wilder_rsi": (ctypes.c_int, [_P, _I64, _I64, _I64, _I32, _P, _I64, _P]),
    "bq_zscore": (ctypes.c_int, [_P, _I64, _I64, _I64, _I32, _P, _I64, _P]),
    "bq_adx": (ctypes.c_int, [_P, _P, _P, _I64, _I64, _I64, _I32, _P, _I64, _P]),
    "bq_micro_regime": (ctypes.c_int, [_I64] + [_P] * 13 + [_P]),
    "bq_symbol_regime_panel": (ctypes.c_int, [_PP, _I64, _P, _I64, _P, _I64, _I64, _I64, _P, _P, _I64, _P, _I64, _P, _P,
                                              _PP, _I64, _PP, _I64, _P]),
    "bq_context_score": (ctypes.c_int, [_I64, _P, _P, _P, _P, ctypes.POINTER(BqContextScalars),
                                        ctypes.POINTER(BqScorerWeights), _P, _I64, _P]),
    "bq_cohort_select": (ctypes.c_int, [_I64, _P, _P, _P, _P, _I32, _P, _P, _P]),
    "bq_parse_kline_events": (ctypes.c_int, [ctypes.c_char_p, _I64, _I64, _P, _I64, _P, _P, _PP, _P, _P, _P]),
}


class NativeLibraryError(RuntimeError):
    pass


_lib: ctypes.CDLL | None = None


def load(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load (once) and type the native library. Raises if it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise NativeLibraryError(
            f"binquant_amd native library not found at {p}; run `make` "
            "(or __graft_entry__.build()) — there is no CPU fallback"
        )
    lib = ctypes.CDLL(str(p), mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # compiled fused programs persist next to the library (bq_fused_jit.hip)
    cache = os.environ.get("BQ_FUSED_CACHE", str(p.parent / "fused_cache"))
    if cache:
        try:
            os.makedirs(cache, exist_ok=True)
            lib.bq_fused_set_cache_dir(cache.encode())
        except OSError:
            pass   # read-only tree: the per-process cache still applies
    if path is None:
        _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status == BQ_OK:
        return
    if status == BQ_EINVAL:
        raise ValueError(f"{what}: invalid argument (status {status})")
    raise RuntimeError(f"{what}: native call failed with status {status}")


def default_params() -> BqParams:
    p = BqParams()
    load().bq_default_params(ctypes.byref(p))
    return p


class BqBurstParams(ctypes.Structure):
    """bq_burst_params (include/binquant_amd.h)"""

    _fields_ = [("volume_multiplier", ctypes.c_double), ("quote_volume_multiplier", ctypes.c_double),
                ("price_threshold", ctypes.c_double), ("min_baseline_volume", ctypes.c_double),
                ("min_range_frac", ctypes.c_double), ("min_body_frac", ctypes.c_double),
                ("max_close_to_high", ctypes.c_double), ("min_recent_up_closes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class BqSpikeParams(ctypes.Structure):
    """bq_spike_params (include/binquant_amd.h)"""

    _fields_ = [("volume_cluster_window", ctypes.c_int32), ("volume_cluster_min_count", ctypes.c_int32),
                ("cumulative_price_window", ctypes.c_int32), ("accel_volume_deriv_window", ctypes.c_int32),
                ("label_mode", ctypes.c_int32), ("require_both_patterns", ctypes.c_int32),
                ("require_bullish_spike", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("cumulative_price_threshold", ctypes.c_double), ("accel_volume_deriv_min", ctypes.c_double),
                ("accel_price_change_min", ctypes.c_double), ("body_size_pct_min", ctypes.c_double)]


def ptr_array(ptrs) -> ctypes.Array:
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, v in enumerate(ptrs):
        arr[i] = v if v else None
    return arr
